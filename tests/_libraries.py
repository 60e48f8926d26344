"""The libraries on the core's public ABI, one row each, and what the tests read from the tree about them.

A row holds only what cannot be read from the tree.  Everything else follows from the name: libneedletail_amd_NAME.so,
include/needletail_amd_NAME.h, csrc/ntk_NAME.hip, and PREFIX / CALLS / SYMBOLS of the binding module.  tests/test_consumer_abi.py
states the checks every row is held to, once; tests/test_NAME_abi.py calls those that are not parametrised there and keeps what is
the library's own.  A new library adds one row here, one CONSUMER line in csrc/Makefile and its entries in the two tables of
__graft_entry__.py: test_three_lists_name_the_same_libraries."""
import ctypes as C
import functools
import importlib
import os
import re
import subprocess
from typing import Callable, NamedTuple, Optional

import pytest

import _builds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "needletail_amd")
CSRC = os.path.join(LIBDIR, "csrc")
INCLUDE = os.path.join(ROOT, "include")
CORE_SO = os.path.join(LIBDIR, "libneedletail_amd.so")
CONSUMER_HPP = ("ntk_consumer.hpp", "ntk_device_mem.hpp", "ntk_chunks.hpp")   # csrc/Makefile CONSUMER_HPP
PRIM = "rocprim::"
ANON = "(anonymous namespace)::"


class Library(NamedTuple):
    name: str
    binding: str                 # needletail_amd.BINDING
    cls: str                     # the public class, in the binding and in needletail_amd.__all__
    calls: tuple                 # the binding's CALLS, in its order: PREFIX + call is every function of the header
    headers: tuple               # csrc headers its object depends on besides CONSUMER_HPP (the Makefile's CONSUMER line)
    example: str                 # examples/EXAMPLE.cpp
    bench: Optional[str]         # tools/BENCH.py
    gpu_tests: str               # the GPU test file, or the file each kernel's test is in
    kernels: dict                # every kernel that is not rocPRIM's -> the GPU test (or (file, test)) that launches it
    leak: str                    # what names a kernel of this library: it matches all of `kernels` and no kernel of another library
    c_main: str                  # the body of main() of a C11 program on the header: struct sizes and constants, 0 if they hold
    no_device: Callable          # nt -> a construction that needs a device
    uses: tuple = ()             # libraries whose public headers its own includes
    links: tuple = ()            # libraries it links besides the core
    prim: Optional[tuple] = ()   # words found among its rocPRIM kernels; None: it ships none
    shape: str = ""              # a stricter form every own kernel has, where the library's test states one
    n_global: Optional[int] = None   # __global__ functions in the source, where the library's test counts them

    so = property(lambda s: os.path.join(LIBDIR, f"libneedletail_amd_{s.name}.so"))
    header = property(lambda s: os.path.join(INCLUDE, f"needletail_amd_{s.name}.h"))
    hip = property(lambda s: os.path.join(CSRC, f"ntk_{s.name}.hip"))
    module = property(lambda s: importlib.import_module("needletail_amd." + s.binding))

    def product_files(self):
        """What ships: the header, the source and its own csrc headers, the binding, the example and the bench tool."""
        return [self.header, self.hip] + [os.path.join(CSRC, h) for h in self.headers] + [
            os.path.join(LIBDIR, self.binding + ".py"), os.path.join(ROOT, "examples", self.example + ".cpp")] + (
            [os.path.join(ROOT, "tools", self.bench + ".py")] if self.bench else [])


def _table(nt):
    return nt.KmerTable(21, nt.PATH_BITS_CANONICAL, 1000)


def _kset(nt):
    return nt.KmerSet.from_arrays([1, 2, 3], [1, 1, 1], 21)


_TABLE_CALLS = ("create", "destroy", "reset", "count_device", "stats", "extract_device", "spectrum", "lookup_device")
_A = ANON
# kmer_sets: <key words, mode (0 COMPARE, 1 COUNT, 2 WRITE), LDS bins of the build>
_JOIN = _A + "ks_join_kernel<{}, {}, {}u>(" + _A + "JoinArgs)"
_SPLIT = _A + "ks_split_kernel<{}>"
_VALIDATE = _A + "ks_validate_kernel<{}>"

LIBRARIES = (
    Library("count", binding="counting", cls="KmerTable", calls=_TABLE_CALLS,
            headers=("ntk_count_common.hpp",), example="count_kmers", bench="count_bench", gpu_tests="test_gpu_count.py", kernels={
        "(anonymous namespace)::kt_insert_kernel((anonymous namespace)::InsertArgs)": ("test_gpu_count.py", "test_random_records_match_the_oracle"),
        "(anonymous namespace)::ct_extract_count_kernel": ("test_gpu_count.py", "test_random_records_match_the_oracle"),
        "(anonymous namespace)::ct_extract_scan_kernel": ("test_gpu_count.py", "test_random_records_match_the_oracle"),
        "(anonymous namespace)::kt_extract_scatter_kernel": ("test_gpu_count.py", "test_random_records_match_the_oracle"),
        "(anonymous namespace)::ct_spectrum_kernel": ("test_gpu_count.py", "test_genome_sampled_reads_spectrum"),
        "(anonymous namespace)::kt_lookup_kernel": ("test_gpu_count.py", "test_golden_28s_and_prjna271013"),
    }, leak=r"(?:^|::)(?:kt|ct)_",
            c_main="return 0;",
            no_device=_table, prim=("radix",)),
    Library("wide_count", binding="wide_counting", cls="WideKmerTable", calls=_TABLE_CALLS,
            headers=("ntk_count_common.hpp",), example="count_kmers", bench="count_bench", gpu_tests="test_gpu_wide_count.py", kernels={
        "(anonymous namespace)::wt_count_kernel((anonymous namespace)::CountArgs)": "test_random_records_match_the_oracle",
        "(anonymous namespace)::ct_extract_count_kernel": "test_random_records_match_the_oracle",
        "(anonymous namespace)::ct_extract_scan_kernel": "test_random_records_match_the_oracle",
        "(anonymous namespace)::wt_extract_scatter_kernel(unsigned long const*, unsigned long const*, unsigned long const*, unsigned long, "
        "unsigned long, unsigned long const*, (anonymous namespace)::WideKey*, unsigned long*)": "test_random_records_match_the_oracle",
        "(anonymous namespace)::ct_spectrum_kernel": "test_synthetic_reads_agree_with_the_reduce_face",
        "(anonymous namespace)::wt_lookup_kernel((anonymous namespace)::Table, unsigned int, unsigned long const*, unsigned long, "
        "unsigned long*)": "test_random_records_match_the_oracle",
    }, leak=r"(?:^|::)(?:wt|ct)_",
            c_main="struct ntk_kmer_table_stats s; (void)s; return 0;",
            no_device=lambda nt: nt.WideKmerTable(51, nt.PATH_BYTES_CANONICAL, 1000), uses=("count",), prim=("radix",)),
    Library("sketch", binding="sketching", cls="KmerSketch", calls=("create", "destroy", "reset", "add_device", "registers", "merge", "estimate"),
            headers=("ntk_wide_walk.hpp",), example="count_kmers", bench="sketch_bench", gpu_tests="test_gpu_sketch.py", kernels={
        "(anonymous namespace)::sk_update_kernel((anonymous namespace)::UpdateArgs)": "test_random_records_match_the_model",
        "(anonymous namespace)::sk_wide_update_kernel((anonymous namespace)::WideArgs)": "test_random_records_match_the_model_wide",
    }, leak=r"(?:^|::)sk_|sketch",
            c_main="struct ntk_kmer_sketch_estimate e; e.capacity = NTK_SKETCH_REGISTERS; "
            "return e.capacity == 16384 && NTK_SKETCH_XOR != 0 ? 0 : 1;",
            no_device=lambda nt: nt.KmerSketch(21, nt.PATH_BITS_CANONICAL), prim=None),
    # bench=None: tools/abundance_bench.py mentions the checker in a comment, so it is the one bench tool not yet held to the rule;
    # once that comment is reworded, name the tool here
    Library("abundance", binding="abundance", cls="ReadAbundance", calls=("create", "destroy", "run_device", "trim"),
            headers=(), example="read_abundance", bench=None, gpu_tests="test_gpu_abundance.py", kernels={
        "(anonymous namespace)::ra_wave_kernel((anonymous namespace)::RaArgs)": "test_random_records_match_the_oracle",
        "(anonymous namespace)::ra_block_kernel((anonymous namespace)::RaArgs)": "test_long_records_on_both_sides_of_the_threshold",
    }, leak=r"(?:^|::)ra_|abundance",
            c_main="struct ntk_read_abundance_row r; r.median = 48; return sizeof r == r.median ? 0 : 1;",
            no_device=lambda nt: nt.ReadAbundance(_table(nt)), uses=("count",), links=("count",), prim=None),
    Library("trim", binding="trimming", cls="ReadTrimmer", calls=("create", "destroy", "release", "run_device", "compact_device"),
            headers=("ntk_trim_runs.hpp",), example="trim_reads", bench="trim_bench", gpu_tests="test_gpu_trim.py", kernels={
        "(anonymous namespace)::rt_solid_kernel((anonymous namespace)::SolidArgs)": "test_random_records_match_the_model",
        "(anonymous namespace)::rt_interval_kernel((anonymous namespace)::IntervalArgs)": "test_random_records_match_the_model",
        "(anonymous namespace)::rt_copy_kernel((anonymous namespace)::CopyArgs)": "test_compaction_matches_the_model",
        "(anonymous namespace)::rt_copy_long_kernel((anonymous namespace)::CopyArgs)": "test_one_record_of_four_million_bases",
    }, leak=r"(?:^|::)rt_|read_trim",
            c_main="struct ntk_read_trim_row r; r.length = 32; return sizeof r == r.length && NTK_TRIM_LONGEST == 1 ? 0 : 1;",
            no_device=lambda nt: nt.ReadTrimmer(_table(nt)), uses=("count",), links=("count",), prim=("scan",), shape=r"::rt_[a-z_]+kernel\("),
    Library("minhash", binding="minhashing", cls="KmerMinHash", calls=("create", "destroy", "reset", "add_device", "stats", "read", "merge", "compare"),
            headers=("ntk_wide_walk.hpp",), example="minhash_sketch", bench="minhash_bench", gpu_tests="test_gpu_minhash.py", kernels={
        "(anonymous namespace)::mh_filter_kernel((anonymous namespace)::FilterArgs)": "test_random_records_match_the_model",
        "(anonymous namespace)::mh_wide_filter_kernel((anonymous namespace)::WideFilterArgs)": "test_random_records_match_the_model_wide",
    }, leak=r"(?:^|::)mh_|minhash",
            c_main="struct ntk_minhash_stats s; struct ntk_minhash_comparison c; s.num = NTK_MINHASH_MAX_NUM; c.dot = 0.0; "
            "return s.num == 1048576 && c.dot == 0.0 && sizeof s == 72 && sizeof c == 56 && NTK_MINHASH_XOR != 0 && "
            "NTK_MINHASH_BUFFER_DEFAULT == 4194304 && NTK_MINHASH_BUFFER_MIN == 64 && NTK_MINHASH_BUFFER_MAX == 268435456 ? 0 : 1;",
            no_device=lambda nt: nt.KmerMinHash(21, nt.PATH_BITS_CANONICAL, num=1000), prim=("sort", "merge", "reduce_by_key"),
            shape=r"::mh_[a-z_]+kernel\("),
    Library("minhash_set", binding="minhash_sets", cls="MinHashSet", calls=("create", "destroy", "reset", "add", "read", "stats", "compare"),
            headers=("ntk_mhset_rank.hpp",), example="minhash_matrix", bench="minhash_set_bench", gpu_tests="test_gpu_minhash_set.py", kernels={
        "(anonymous namespace)::ms_cut_kernel((anonymous namespace)::CutArgs)": "test_block_matches_the_host_compare",
        "(anonymous namespace)::ms_pair_kernel((anonymous namespace)::PairArgs)": "test_block_matches_the_host_compare",
    }, leak=r"(?:^|::)ms_",
            c_main="struct ntk_mhset_stats s; s.n_sketches = NTK_MHSET_BLOCK_MAX; "
            "return s.n_sketches == 67108864 && sizeof s == 56 && sizeof(struct ntk_mhset_stats) == 56 && "
            "NTK_MHSET_BLOCK_DEFAULT == 1048576 && NTK_MHSET_BLOCK_MIN == 1 && NTK_MHSET_STAGE == 2048 ? 0 : 1;",
            no_device=lambda nt: nt.MinHashSet(), prim=None, shape=r"::ms_(?:cut|pair)_kernel\(", n_global=2),
    Library("record_minhash", binding="record_minhashing", cls="RecordMinHash", calls=("create", "destroy", "run_device", "read", "stats", "trim"),
            headers=("ntk_rmh_rule.hpp",), example="sketch_records", bench="record_minhash_bench", gpu_tests="test_gpu_record_minhash.py", kernels={
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
    }, leak=r"(?:^|::)rmh_",
            c_main="struct ntk_record_minhash_stats s; s.n_records = "
            "NTK_RECORD_MINHASH_BUFFER_MAX; return s.n_records == 1073741824 && sizeof s == 88 && NTK_RECORD_MINHASH_ALLPASS == 4 && "
            "NTK_RECORD_MINHASH_BUFFER_DEFAULT == 16777216 && NTK_RECORD_MINHASH_BUFFER_MIN == 256 && "
            "NTK_RECORD_MINHASH_MAX_NUM == 1048576 && NTK_RECORD_MINHASH_XOR == 0x9E3779B97F4A7C15ull ? 0 : 1;",
            no_device=lambda nt: nt.RecordMinHash(21, nt.PATH_BYTES_CANONICAL, num=16), prim=("sort", "scan"), shape=r"::rmh_[a-z_]+_kernel\b",
            n_global=10),
    Library("kmer_sets", binding="kmer_sets", cls="KmerSet", calls=("create", "destroy", "release", "stats", "validate_device", "compare_device", "apply_device"),
            headers=("ntk_kset_rule.hpp",), example="compare_tables", bench="kmer_sets_bench", gpu_tests="test_gpu_kmer_sets.py", kernels={
        _SPLIT.format(1): "test_lengths_around_the_tile_seams", _SPLIT.format(2): "test_lengths_around_the_tile_seams",
        _VALIDATE.format(1): "test_validate_counts_a_swapped_pair_and_a_duplicate",
        _VALIDATE.format(2): "test_validate_counts_a_swapped_pair_and_a_duplicate",
        _JOIN.format(1, 0, 4096): "test_lengths_around_the_tile_seams", _JOIN.format(2, 0, 4096): "test_lengths_around_the_tile_seams",
        _JOIN.format(1, 0, 16384): "test_counts_at_below_and_above_the_last_bin", _JOIN.format(2, 0, 16384): "test_key_edges_wide",
        _JOIN.format(1, 1, 1): "test_capacity_query_exact_fit_and_one_short", _JOIN.format(2, 1, 1): "test_capacity_query_exact_fit_and_one_short",
        _JOIN.format(1, 2, 1): "test_every_op_and_rule_on_random_lists", _JOIN.format(2, 2, 1): "test_every_op_and_rule_on_random_lists",
    }, leak=r"(?:^|::)ks_",
            c_main="struct ntk_kmer_sets_totals t; struct ntk_kmer_sets_stats s; "
            "t.sum_max = NTK_KSET_MAX_BINS; s.n_calls = NTK_KSET_TILE_WORDS; "
            "return t.sum_max == 16384 && s.n_calls == 2048 && sizeof t == 104 && sizeof s == 32 && NTK_KSET_INTERSECT == 1 && "
            "NTK_KSET_UNION == 2 && NTK_KSET_SUBTRACT == 3 && NTK_KSET_COUNTERS_SUBTRACT == 4 && NTK_KSET_MIN == 1 && NTK_KSET_MAX == 2 && "
            "NTK_KSET_SUM == 3 && NTK_KSET_LEFT == 4 && NTK_KSET_RIGHT == 5 ? 0 : 1;",
            no_device=_kset,
            shape=r"::ks_(?:split|join|validate)_kernel<", n_global=3),
    Library("dbg", binding="dbg", cls="KmerGraph", calls=("create", "destroy", "release", "stats", "adjacency_device", "unitigs_device", "spell_device"),
            headers=("ntk_dbg_rule.hpp",), example="unitigs", bench="dbg_bench", gpu_tests="test_gpu_dbg.py", kernels={
        "dbg_dir_mark_kernel": "test_directory_with_empty_buckets_and_with_one_bucket",
        "dbg_adjacency_kernel": "test_subsets_of_3_mers_and_5_mers",
        "dbg_link_kernel": "test_subsets_of_3_mers_and_5_mers",
        "dbg_rank_init_kernel": "test_a_long_path_needs_its_rounds",
        "dbg_rank_round_kernel": "test_a_long_path_needs_its_rounds",
        "dbg_rank_cut_kernel": "test_the_same_sequence_as_a_cycle",
        "dbg_resolve_kernel": "test_subsets_of_3_mers_and_5_mers",
        "dbg_perm_kernel": "test_subsets_of_3_mers_and_5_mers",
        "dbg_rows_kernel": "test_subsets_of_3_mers_and_5_mers",
        "dbg_spell_kernel": "test_subsets_of_3_mers_and_5_mers",
    }, leak=r"(?:^|::)dbg_",
            c_main="struct ntk_dbg_totals t; struct ntk_dbg_stats s; struct ntk_dbg_kmer_row kr; "
            "struct ntk_dbg_unitig_row ur; t.deg_hist[4][4] = NTK_DBG_K_MAX; s.n_rounds = NTK_DBG_K_MIN; kr.pos_flip = 1; ur.flags = NTK_DBG_FLAG_CYCLE; "
            "return sizeof t == 248 && sizeof s == 40 && sizeof kr == 8 && sizeof ur == 32 && t.deg_hist[4][4] == 31 && s.n_rounds == 3 && "
            "kr.pos_flip == ur.flags && NTK_DBG_N_MAX == 2147483647 && NTK_DBG_UNITIG_BYTES_PER_KMER == 96 ? 0 : 1;",
            no_device=lambda nt: nt.KmerGraph(_kset(nt)), n_global=10),
)
BY_NAME = {lib.name: lib for lib in LIBRARIES}
# the one family of kernels two libraries own together: the extract count / scan and spectrum kernels of ntk_count_common.hpp
SHARED_KERNELS = ({"count", "wide_count"}, r"(?:^|::)ct_")


def built(path=CORE_SO):
    """`path`, a built library: the libraries are built first if it is not there."""
    if not os.path.exists(path):
        subprocess.check_call(["make", "-s", "-C", CSRC])
    return path


def no_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def header_symbols(path):
    """The ntk_* functions a C header declares."""
    hdr = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(ntk_[a-z0-9_]+)\s*\(", hdr)))


def own_kernels(names):
    return {n for n in names if not n.startswith(PRIM)}


def bare(kernel):
    """`(anonymous namespace)::dbg_rows_kernel((anonymous namespace)::RowsArgs)` -> `dbg_rows_kernel`."""
    return re.sub(r"^\(anonymous namespace\)::", "", kernel).split("(")[0]


class MakeDatabase(NamedTuple):
    prerequisites: dict   # target -> the set of its prerequisites, after expansion
    variables: dict       # name -> value as the Makefile states it
    build: list           # the command lines of `make -n -B`
    clean: list           # the command lines of `make -n clean`


@functools.lru_cache(maxsize=None)
def make_database():
    """csrc/Makefile as make reads it: nothing is built."""
    run = lambda *args: subprocess.run(["make", "-n", "-C", CSRC, "ARCH=gfx950", *args], capture_output=True, text=True, check=True).stdout   # noqa: E731
    commands, files = run("-B", "-p").split("# Files", 1)
    prerequisites = {}
    for m in re.finditer(r"^([^\s#:=][^:=\n]*):(?!=)([^\n]*)$", files, re.M):
        prerequisites.setdefault(m.group(1).strip(), set()).update(m.group(2).split())
    variables = dict(re.findall(r"^(\w+) :?= (.*)$", commands, re.M))
    lines = lambda out: [ln for ln in out.splitlines() if ln and not ln.startswith(("make", "#"))]   # noqa: E731
    return MakeDatabase(prerequisites, variables, lines(commands.split("# Make data base", 1)[0]), lines(run("clean")))


def so_path(name):
    return os.path.join(LIBDIR, f"libneedletail_amd_{name}.so" if name else "libneedletail_amd.so")


def public_header(name):
    return "../../include/needletail_amd%s.h" % ("_" + name if name else "")


# ---- the checks every row is held to that tests/test_NAME_abi.py calls with its row (the others: tests/test_consumer_abi.py) --------

def check_exports(row):
    """Declared in the header = listed by the binding = exported by the library, and nothing else under the project's prefix."""
    lib, mod = C.CDLL(built(row.so)), row.module
    syms = header_symbols(row.header)
    assert syms == sorted(mod.PREFIX + c for c in row.calls) and list(mod.CALLS) == list(row.calls)
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in {os.path.basename(row.header)} but not exported"
    assert sorted(mod.SYMBOLS) == syms
    exported = subprocess.run(["nm", "-D", "--defined-only", row.so], capture_output=True, text=True).stdout
    assert sorted(set(re.findall(r"\b(ntk_\w+)", exported))) == syms, "nothing else is exported under the project's prefix"
    import needletail_amd as nt
    assert getattr(nt, row.cls) is getattr(mod, row.cls) and row.cls in nt.__all__
    assert mod.LIB_PATH == row.so


def check_header(row, tmp_path):
    """A C11 program on the header compiles, links and states the struct sizes and constants; what the header includes."""
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text(f'#include "{os.path.basename(row.header)}"\nint main(void) {{ {row.c_main} }}\n')
    r = subprocess.run(["gcc", "-std=c11", "-pedantic", "-Wall", "-Werror", "-I" + INCLUDE, "-o", str(exe), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert subprocess.run([str(exe)]).returncode == 0, "a struct size or a constant is not the stated one"
    includes = lambda path: re.findall(r'#include\s+[<"]([^>"]+)[>"]', open(path).read())   # noqa: E731
    assert includes(row.header) == [os.path.basename(public_header(row.uses[0] if row.uses else ""))]
    # followed through, they are the public headers the Makefile's object rule names: the library's, those it calls and the core's
    seen, todo = set(), [os.path.basename(row.header)]
    while todo:
        h = todo.pop()
        if h not in seen and os.path.exists(os.path.join(INCLUDE, h)):
            seen.add(h)
            todo += includes(os.path.join(INCLUDE, h))
    named = {os.path.basename(p) for p in make_database().prerequisites[f"ntk_{row.name}.o"] if p.startswith("../../include/")}
    assert seen == named == {os.path.basename(public_header(n)) for n in (row.name, "") + row.uses}


def check_kernels(row):
    """Its kernels that are not rocPRIM's are the row's, each with a GPU test that exists; the shape, rocPRIM words and counts the row states."""
    names = _builds.library_kernels(built(row.so))
    ours = own_kernels(names)
    assert {n if n in row.kernels else bare(n) for n in ours} == set(row.kernels) and len(ours) == len(row.kernels), sorted(ours)
    assert all(re.search(row.shape, n) for n in ours)
    if row.prim is None:
        assert names == ours, "the library ships no rocPRIM kernel"
    for word in row.prim or ():
        assert any(word in n for n in names - ours), word
    for sym, test in row.kernels.items():
        fname, test = test if isinstance(test, tuple) else (row.gpu_tests, test)
        assert re.search(rf"^def {re.escape(test)}\(", open(os.path.join(ROOT, "tests", fname)).read(), re.M), (sym, fname, test)
    if row.n_global is not None:
        assert len(re.findall(r"__global__", open(row.hip).read())) == row.n_global


def check_product_files_never_name_the_checker(row):
    for path in row.product_files():
        assert not re.search(r"\boracle\b|ntko_", open(path).read()), path


def check_no_device(row, skip=True):
    """Without a GPU the row's construction is NTK_ERR_NO_DEVICE; with one there is nothing to check here."""
    import torch
    if torch.cuda.is_available():
        if skip:
            pytest.skip("GPU present")
        return
    import needletail_amd as nt
    from needletail_amd import engine
    row.module.lib()   # the library itself loads without a device
    engine._default_ctx = None
    with pytest.raises(nt.NtkError) as e:
        row.no_device(nt)
    assert e.value.status == 4   # NTK_ERR_NO_DEVICE
