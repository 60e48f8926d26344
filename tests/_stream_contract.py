"""The stream contract of the device face, call by call: one row per exported function of include/needletail_amd.h, the eleven
include/needletail_amd_*.h and include/needletail_amd/minimizer_list.h that takes a device pointer or queues work on the context's stream.  tests/test_stream_contract.py holds the
rows to the headers; tests/test_gpu_stream_order.py holds the calls to the rows.

A row's class is what the header promises about the context's stream:
  ASYNC     the call queues its work and returns; it neither waits for the stream nor reads what the stream has not produced yet.  (A
            call that only changes host-side state - ntk_accum_bind_device, ntk_accum_device_ptr - is of this class: it queues nothing
            and waits for nothing.)  The one exception is what ntk_device_mem.hpp calls THE ONE RULE: a call whose scratch has to grow
            synchronises before the old array is freed.
  MAY_SYNC  the call may or may not wait for the stream; its result is ordered on the stream either way.
  SYNC      the stream is drained when the call returns: outputs are written, host results are final.
`words` are the header's own, quoted; `where` says whether they stand at the declaration ("decl": in the comment in front of it or on its
line) or in the comment at the head of the file, which then names the call ("head").  `test` is the GPU test that makes the call with work
pending: of tests/test_gpu_stream_order.py, or of the file the row names in `file`.

Out of scope, in one line: the compat face (host arrays in, host arrays out; "eager, synchronous"), the readers and the whole-file
pipelines, the option / timing / communicator calls, create / destroy / release, and ntk_batch_acquire / append / buffers / wait / release
(host work on pinned memory; ntk_batch_wait is exercised beside ntk_batch_submit)."""
import collections
import os
import re

ASYNC, MAY_SYNC, SYNC = "ASYNC", "MAY_SYNC", "SYNC"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
GPU_TESTS = "test_gpu_stream_order.py"

HEADERS = ("needletail_amd.h", "needletail_amd_count.h", "needletail_amd_wide_count.h", "needletail_amd_sketch.h", "needletail_amd_minhash.h",
           "needletail_amd_abundance.h", "needletail_amd_trim.h", "needletail_amd_record_minhash.h", "needletail_amd_minhash_set.h",
           "needletail_amd_kmer_sets.h", "needletail_amd_dbg.h", "needletail_amd_colors.h", "needletail_amd/minimizer_list.h")

Row = collections.namedtuple("Row", "function cls header words where test file", defaults=(GPU_TESTS,))

_CORE, _COUNT, _WIDE, _SKETCH, _MINHASH, _ABUND, _TRIM, _RMH, _MHSET, _KSETS, _DBG, _COLORS, _ML = HEADERS
_TABLE_HEAD = "stats, extract, spectrum and lookup synchronise it"
_KSETS_HEAD = "Every call returns a status code of needletail_amd.h and is synchronous on the context's stream"
_ML_HEAD = "run_device, read, stats and trim are SYNCHRONOUS: they return when the work they queued on the context's stream is done"
_ML_TESTS = "test_gpu_minimizer_list.py"


def _table_rows(prefix, header):
    return [
        Row(prefix + "reset", ASYNC, header, "Empties the table (async).", "decl", "test_count_table"),
        Row(prefix + "count_device", ASYNC, header, "(async)", "decl", "test_count_table"),
        Row(prefix + "stats", SYNC, header, "Synchronises.", "decl", "test_count_table"),
        Row(prefix + "extract_device", SYNC, header, _TABLE_HEAD, "head", "test_kmer_sets"),
        Row(prefix + "spectrum", SYNC, header, _TABLE_HEAD, "head", "test_count_table"),
        Row(prefix + "lookup_device", SYNC, header, _TABLE_HEAD, "head", "test_count_table"),
    ]


ROWS = [
    # the core
    Row("ntk_accum_reset", ASYNC, _CORE, "async: the zeroing is queued on the ctx stream", "decl", "test_accum_reset_ahead_of_a_reduce"),
    Row("ntk_reduce_device", ASYNC, _CORE, "/* async */", "decl", "test_reduce_device"),
    Row("ntk_reduce_device_quality", ASYNC, _CORE, "/* async */", "decl", "test_reduce_device"),
    Row("ntk_accum_read", SYNC, _CORE, "synchronises the ctx stream", "decl", "test_reduce_device"),
    Row("ntk_accum_device_ptr", ASYNC, _CORE, "host-side only: queues nothing and waits for nothing", "decl", "test_accum_bind_device"),
    Row("ntk_accum_bind_device", ASYNC, _CORE, "Host-side only: queues nothing and waits for nothing", "decl", "test_accum_bind_device"),
    Row("ntk_materialize_device", ASYNC, _CORE, "/* async */", "decl", "test_materialize_device"),
    Row("ntk_materialize_device_quality", ASYNC, _CORE, "/* async */", "decl", "test_materialize_device"),
    Row("ntk_batch_submit", ASYNC, _CORE, "async: H2D + reduce", "decl", "test_batch_submit_behind_pending_work"),
    Row("ntk_minimizers_reduce_device", ASYNC, _CORE, "Async on the ctx stream.", "decl", "test_minimizers_reduce_device"),
    Row("ntk_synth_reads_device", ASYNC, _CORE, "Async on the ctx stream.", "decl", "test_synth_reads_device_into_a_reduce"),
    Row("ntk_reverse_complement_records_device", ASYNC, _CORE, "Async on the ctx stream.", "decl", "test_reverse_complement_records_device"),
    # the two count tables
    *_table_rows("ntk_kmer_table_", _COUNT),
    *_table_rows("ntk_wide_table_", _WIDE),
    # the HyperLogLog sketch
    Row("ntk_kmer_sketch_reset", ASYNC, _SKETCH, "(async)", "decl", "test_kmer_sketch"),
    Row("ntk_kmer_sketch_add_device", ASYNC, _SKETCH, "Adds every k-mer the batch emits (async)", "decl", "test_kmer_sketch"),
    Row("ntk_kmer_sketch_registers", SYNC, _SKETCH, "(synchronises)", "decl", "test_kmer_sketch"),
    Row("ntk_kmer_sketch_merge", SYNC, _SKETCH, "(synchronises)", "decl", "test_merges_from_host_arrays"),
    Row("ntk_kmer_sketch_estimate", SYNC, _SKETCH, "(synchronises)", "decl", "test_kmer_sketch"),
    # MinHash
    Row("ntk_minhash_reset", ASYNC, _MINHASH, "(async)", "decl", "test_minhash_add_device"),
    Row("ntk_minhash_add_device", MAY_SYNC, _MINHASH, "(may synchronise the stream)", "decl", "test_minhash_add_device"),
    Row("ntk_minhash_stats", SYNC, _MINHASH, "(synchronises)", "decl", "test_minhash_add_device"),
    Row("ntk_minhash_read", SYNC, _MINHASH, "(synchronises)", "decl", "test_minhash_add_device"),
    Row("ntk_minhash_merge", SYNC, _MINHASH, "(synchronises)", "decl", "test_merges_from_host_arrays"),
    # abundance, trim
    Row("ntk_read_abundance_run_device", SYNC, _ABUND, "Synchronous: the call returns after the rows are written", "decl", "test_read_abundance"),
    Row("ntk_read_trim_run_device", SYNC, _TRIM, "Synchronous: the call returns after the rows are written", "decl", "test_read_trim_and_compact"),
    Row("ntk_read_trim_compact_device", SYNC, _TRIM, "Synchronous.", "decl", "test_read_trim_and_compact"),
    # per-record MinHash
    Row("ntk_record_minhash_run_device", SYNC, _RMH, "(synchronous)", "decl", "test_record_minhash"),
    Row("ntk_record_minhash_read", SYNC, _RMH, "(synchronous)", "decl", "test_record_minhash"),
    Row("ntk_record_minhash_stats", SYNC, _RMH, "(synchronous)", "decl", "test_record_minhash"),
    Row("ntk_record_minhash_trim", SYNC, _RMH, "(synchronous)", "decl", "test_record_minhash"),
    # the sketch set
    Row("ntk_mhset_read", SYNC, _MHSET, "(synchronises)", "decl", "test_mhset_compare"),
    Row("ntk_mhset_compare", SYNC, _MHSET, "(synchronises)", "decl", "test_mhset_compare"),
    # k-mer set algebra, the graph
    Row("ntk_kmer_sets_validate_device", SYNC, _KSETS, _KSETS_HEAD, "head", "test_kmer_sets"),
    Row("ntk_kmer_sets_compare_device", SYNC, _KSETS, _KSETS_HEAD, "head", "test_kmer_sets"),
    Row("ntk_kmer_sets_apply_device", SYNC, _KSETS, _KSETS_HEAD, "head", "test_kmer_sets"),
    Row("ntk_dbg_adjacency_device", SYNC, _DBG, _KSETS_HEAD, "head", "test_dbg"),
    Row("ntk_dbg_unitigs_device", SYNC, _DBG, _KSETS_HEAD, "head", "test_dbg"),
    Row("ntk_dbg_spell_device", SYNC, _DBG, _KSETS_HEAD, "head", "test_dbg"),
    # the coloured index
    Row("ntk_kmer_colors_reset", ASYNC, _COLORS, "queued on the stream", "decl", "test_kmer_colors_add"),
    Row("ntk_kmer_colors_add_device", ASYNC, _COLORS, "Queued on the stream.", "decl", "test_kmer_colors_add"),
    Row("ntk_kmer_colors_stats", SYNC, _COLORS, "Synchronises", "decl", "test_kmer_colors_add"),
    Row("ntk_kmer_colors_lookup_device", SYNC, _COLORS, "Synchronous.", "decl", "test_kmer_colors_run_and_lookup"),
    Row("ntk_kmer_colors_run_device", SYNC, _COLORS, "Synchronous: the call returns after everything is written.", "decl", "test_kmer_colors_run_and_lookup"),
    # the minimizer lists: the library's own GPU file makes the calls with work pending
    Row("ntk_minimizer_list_run_device", SYNC, _ML, _ML_HEAD, "head", "test_stream_order", _ML_TESTS),
    Row("ntk_minimizer_list_read", SYNC, _ML, _ML_HEAD, "head", "test_stream_order", _ML_TESTS),
    Row("ntk_minimizer_list_result_device", ASYNC, _ML, "host-side only: queues nothing and waits for nothing", "decl", "test_stream_order", _ML_TESTS),
    Row("ntk_minimizer_list_stats", SYNC, _ML, _ML_HEAD, "head", "test_stream_order", _ML_TESTS),
    Row("ntk_minimizer_list_trim", SYNC, _ML, _ML_HEAD, "head", "test_stream_order", _ML_TESTS),
]

# calls without a device pointer that the headers' contract sentences name: they queue work on the context's stream or wait for it
NAMED = ("ntk_accum_reset", "ntk_accum_read", "ntk_batch_submit",
         "ntk_kmer_table_reset", "ntk_kmer_table_stats", "ntk_kmer_table_spectrum", "ntk_wide_table_reset", "ntk_wide_table_stats", "ntk_wide_table_spectrum",
         "ntk_kmer_sketch_reset", "ntk_kmer_sketch_registers", "ntk_kmer_sketch_merge", "ntk_kmer_sketch_estimate",
         "ntk_minhash_reset", "ntk_minhash_stats", "ntk_minhash_read", "ntk_minhash_merge",
         "ntk_record_minhash_read", "ntk_record_minhash_stats", "ntk_record_minhash_trim", "ntk_mhset_read", "ntk_mhset_compare",
         "ntk_kmer_colors_reset", "ntk_kmer_colors_stats",
         "ntk_minimizer_list_read", "ntk_minimizer_list_stats", "ntk_minimizer_list_trim")


def shipped_headers() -> list:
    """Every .h below include/, as a path relative to it: the walk is recursive, so a header in a directory of its own is seen too."""
    out = []
    for folder, _, files in os.walk(INCLUDE):
        out += [os.path.relpath(os.path.join(folder, f), INCLUDE).replace(os.sep, "/") for f in files if f.endswith(".h")]
    return sorted(out)


def header_text(name: str) -> str:
    with open(os.path.join(INCLUDE, name)) as f:
        return f.read()


def plain(text: str) -> str:
    """Comment text as prose: the frames of a block comment and the line breaks inside a sentence are not part of the words."""
    text = re.sub(r"^\s*\* ?", " ", text, flags=re.M)
    return re.sub(r"\s+", " ", text)


def declarations(text: str):
    """(name, parameter text, the comment text next to it) of every `int ntk_*(` declaration: next to it is what stands between the end
    of the declaration before it (or the end of that one's line) and the end of its own line."""
    out, last = [], 0
    for m in re.finditer(r"^int (ntk_\w+)\(", text, re.M):
        end = text.index(";", m.end())
        params = re.sub(r"/\*.*?\*/", " ", text[m.end():end], flags=re.S)
        line_end = text.find("\n", end)
        line_end = len(text) if line_end < 0 else line_end
        out.append((m.group(1), params, text[last:m.start()] + " " + text[end:line_end]))
        last = line_end
    return out


def head_comment(text: str) -> str:
    """The comment at the head of the file."""
    return text[:text.index("*/") + 2]


def takes_device_pointer(params: str) -> bool:
    return re.search(r"\bd_\w+", params) is not None


def table_markdown() -> str:
    lines = ["| call | class | header | the header's words | GPU test |", "|---|---|---|---|---|"]
    for r in ROWS:
        lines.append(f"| `{r.function}` | {r.cls} | `{r.header}` ({r.where}) | \"{r.words.replace('/*', '').replace('*/', '').strip()}\" | `{r.test if r.file == GPU_TESTS else r.file + '::' + r.test}` |")
    return "\n".join(lines)
