"""Every launch of the twelve k-mer libraries whose grid is capped by the device's CU count, one row each, and the GPU test that takes
the kernel past one step of its grid-stride loop.

A capped launch is `grid_for(items, per_block, n_cu * C)`: min(ceil(items / per_block), n_cu * C) blocks, each walking the items in
steps of gridDim * per_block.  A fixed launch is `dim3(n_cu * C)`.  Either way one step of the whole grid takes
`items_per_step(row, cu) = per_block * C * cu` items, and a kernel whose input is not larger than that has run its loop body once.
tests/test_grid_steps.py holds every row to the text of its source; tests/test_gpu_grid_steps.py sizes its inputs from the rows and
the device's CU count."""
import os
from typing import NamedTuple, Optional

import _libraries as L

COLORS_FILES = ("ntk_colors.hip", "ntk_colors_rule.hpp")
ML_FILES = ("ntk_minimizer_list.hip", "ntk_ml_rule.hpp")
ML_TESTS = "test_gpu_minimizer_list.py"
NEW = "test_gpu_grid_steps.py"


def files_of(lib: str) -> tuple:
    """The csrc files that hold the library's launches: its source and its own headers."""
    if lib == "colors":
        return COLORS_FILES
    if lib == "minimizer_list":
        return ML_FILES
    return (f"ntk_{lib}.hip",) + tuple(L.BY_NAME[lib].headers)


LIBS = tuple(row.name for row in L.LIBRARIES) + ("colors", "minimizer_list")

# what the items of some rows are worth, for the arithmetic in the notes (tests/test_grid_steps.py ties them too)
K_LANE_RUN = ("ntk_wide_walk.hpp", "kLaneRun", 64)         # bytes per run of the k > 32 walkers
K_PER_LANE = (("ntk_sketch.hip", "kPerLane", 4), ("ntk_minhash.hip", "kPerLane", 4), ("ntk_record_minhash.hip", "kPerLane", 4))
K_CHUNK = 64 << 20                                          # kChunkBases (tests/test_count_abi.py ties it)
K_RMH_SEGMENT = 4 * 64 * 4 * 4                              # kSegment of ntk_record_minhash.hip: 4 * kTile * 4, kTile = 64 * kPerLane
K_ML_TILE = ("ntk_ml_rule.hpp", "ML_TILE", 1024)            # window ends per tile of the two tile kernels of ntk_minimizer_list.hip


class Row(NamedTuple):
    lib: str
    kernel: str
    item: str                    # what one item of the stride is
    file: str                    # where the launch is
    site: str                    # the grid expression, as the source writes it
    per_block: int               # items a block takes per step ...
    per_block_text: str          # ... and how the source writes it (inside `site` for a capped launch)
    factor: Optional[int]        # blocks per CU; None: the cap is 2^31 - 1 blocks, which no list reaches
    cap_text: str                # how the source writes the cap
    grid: str                    # "capped": grid_for; "fixed": that many blocks whatever the input
    test: Optional[tuple]        # (file, test) of the GPU test that takes it past one step; None where none can (see `note`)
    note: str                    # the arithmetic at 256 CUs
    launch: str = ""             # where the site is not in the launch statement: a regex of the launches it reaches, group 1 the kernel
    cap_def: str = ""            # where the cap is a local: the statement that defines it
    also: Optional[tuple] = None # a second test: the new one, where `test` is one the suite had before; or the one-step pair


def _capped(lib, kernel, item, file, items_text, per_block, per_block_text, factor, cap_text, test, note, **kw):
    return Row(lib, kernel, item, file, f"grid_for({items_text}, {per_block_text}, {cap_text})", per_block, per_block_text, factor, cap_text,
               "capped", test, note, **kw)


def _fixed(lib, kernel, item, file, per_block, per_block_text, factor, cap_text, test, note, **kw):
    return Row(lib, kernel, item, file, f"dim3({cap_text})", per_block, per_block_text, factor, cap_text, "fixed", test, note, **kw)


_DBG = dict(launch=r"DBG_LAUNCH\(h, (dbg_\w+_kernel),")
_DBG_TEST = (NEW, "test_dbg_lists_take_a_second_step")


_DBG_PAIR = (NEW, "test_dbg_adjacency_at_one_step_and_one_more")   # exactly one step of k-mers, and one more: the adjacency call's kernels


def _dbg(kernel, item, note, also=None):
    return _capped("dbg", kernel, item, "ntk_dbg.hip", "items", 256, "kThreads", 16, "(unsigned)n_cu * kBlocksPerCu", _DBG_TEST, note,
                   also=also, **_DBG)


_N = "2^20 k-mers per step; 1.25 x 2^20 keys"
_S = "2^20 states (2 per k-mer) per step; 2.5 x 2^20 states"

ROWS = (
    # ---- count: the per-base kernels run once per chunk of 64 Mi bases, so a batch above a chunk is 128 steps at 256 CUs ----------------
    _capped("count", "kt_insert_kernel", "window ends of a chunk", "ntk_count.hip", "a.n - a.first", 256, "kThreads", 8, "(unsigned)t->n_cu * 8",
            ("test_gpu_count.py", "test_chunk_boundaries_are_counted_once"), "524 288 ends per step; 75.5 M bases, chunks of 64 Mi: 128 steps"),
    _capped("count", "kt_lookup_kernel", "queries", "ntk_count.hip", "n", 256, "kThreads", 8, "(unsigned)t->n_cu * 8",
            ("test_gpu_abundance.py", "test_a_record_longer_than_a_chunk"),
            "524 288 queries per step; the abundance call looks up a chunk's 64 Mi values at once: 128 steps"),
    _capped("count", "ct_spectrum_kernel", "slots", "ntk_count_common.hpp", "slots", 256, "kThreads", 2, "(unsigned)n_cu * 2",
            ("test_gpu_count.py", "test_genome_sampled_reads_spectrum"), "131 072 slots per step; capacity 2.1 M is 2^22 slots: 32 steps"),
    # ---- wide_count ----------------------------------------------------------------------------------------------------------------------
    _capped("wide_count", "wt_count_kernel", "runs of 64 bytes", "ntk_wide_count.hip", "runs", 256, "kThreads", 8, "(unsigned)t->n_cu * 8",
            ("test_gpu_wide_count.py", "test_more_than_2_32_bytes_in_one_call"), "524 288 runs = 32 MiB per step; 4.3 GB: 129 steps"),
    _capped("wide_count", "wt_lookup_kernel", "queries", "ntk_wide_count.hip", "n", 256, "kThreads", 8, "(unsigned)t->n_cu * 8",
            (NEW, "test_wide_lookup_takes_a_second_step"), "524 288 queries per step; the suite's largest query list was a few thousand"),
    _capped("wide_count", "ct_spectrum_kernel", "slots", "ntk_count_common.hpp", "slots", 256, "kThreads", 2, "(unsigned)n_cu * 2",
            ("test_gpu_wide_count.py", "test_synthetic_reads_agree_with_the_reduce_face"),
            "131 072 slots per step; a table of 1 M reads x 100 windows has 2^27 slots or more: 1 024 steps"),
    # ---- sketch --------------------------------------------------------------------------------------------------------------------------
    _capped("sketch", "sk_update_kernel", "rounds of 4 window ends", "ntk_sketch.hip", "rounds", 1024, "kSketchThreads", 2, "resident",
            ("test_gpu_sketch.py", "test_chunk_boundaries_are_taken_once"), "524 288 rounds = 2 Mi ends per step; a chunk of 64 Mi: 32 steps",
            cap_def="const unsigned resident = (unsigned)s->n_cu * 2;"),
    _capped("sketch", "sk_wide_update_kernel", "runs of 64 bytes", "ntk_sketch.hip", "runs", 1024, "kSketchThreads", 2, "resident",
            ("test_gpu_sketch.py", "test_one_key_2_26_times"), "524 288 runs = 32 MiB per step; 2^26 bytes at k = 51: 2 whole steps",
            cap_def="const unsigned resident = (unsigned)s->n_cu * 2;"),
    # ---- abundance -----------------------------------------------------------------------------------------------------------------------
    _capped("abundance", "ra_wave_kernel", "records", "ntk_abundance.hip", "n_records", 4, "kWaveThreads / 64", 8, "(unsigned)a->n_cu * 8",
            (NEW, "test_abundance_records_take_a_second_step"), "8 192 records per step; 10 240 records"),
    _fixed("abundance", "ra_block_kernel", "records of more than 65 536 windows", "ntk_abundance.hip", 1, "1", 1, "(unsigned)a->n_cu",
           (NEW, "test_abundance_long_records_take_a_second_step"), "256 long records per step; 320 long records"),
    # ---- trim ----------------------------------------------------------------------------------------------------------------------------
    _capped("trim", "rt_solid_kernel", "window ends of a chunk", "ntk_trim.hip", "g.n", 1024, "64 * kSolidRounds * (kSolidThreads / 64)", 8,
            "(unsigned)t->n_cu * 8", ("test_gpu_trim.py", "test_a_batch_above_a_chunk_with_weak_windows_around_the_seam"),
            "2 Mi ends per step; a chunk of 64 Mi: 32 steps"),
    _capped("trim", "rt_interval_kernel", "records", "ntk_trim.hip", "n_records", 32, "(64 / kGroup) * (kIntervalThreads / 64)", 8,
            "(unsigned)t->n_cu * 8", (NEW, "test_trim_records_take_a_second_step"), "65 536 records per step; 81 920 records"),
    _capped("trim", "rt_copy_kernel", "records", "ntk_trim.hip", "n_records", 16, "kCopyThreads / kCopyGroup", 8, "(unsigned)t->n_cu * 8",
            (NEW, "test_trim_records_take_a_second_step"), "32 768 records per step; 81 920 records: 3 steps"),
    _fixed("trim", "rt_copy_long_kernel", "16-byte pieces of one long record", "ntk_trim.hip", 256, "kCopyThreads", 4, "(unsigned)t->n_cu * 4",
           ("test_gpu_trim.py", "test_one_record_of_four_million_bases"), "262 144 pieces per step; 2^22 + 1000 bases are 262 207 pieces"),
    # ---- minhash -------------------------------------------------------------------------------------------------------------------------
    _capped("minhash", "mh_filter_kernel", "rounds of 4 window ends", "ntk_minhash.hip", "rounds", 256, "kFilterThreads", 8, "resident",
            ("test_gpu_minhash.py", "test_chunk_boundaries_are_taken_once"),
            "524 288 rounds = 2 Mi ends per step; a scaled sketch takes a chunk of 64 Mi in one launch: 32 steps",
            cap_def="const unsigned resident = (unsigned)m->n_cu * kBlocksPerCu;"),
    _capped("minhash", "mh_wide_filter_kernel", "runs of 64 bytes", "ntk_minhash.hip", "hi - lo", 256, "kFilterThreads", 8, "resident",
            (NEW, "test_wide_minhash_takes_a_second_step"),
            "524 288 runs = 32 MiB per step (a scaled sketch: one launch); the suite's largest k > 32 input was 1 MiB",
            cap_def="const unsigned resident = (unsigned)m->n_cu * kBlocksPerCu;"),
    # ---- minhash_set ---------------------------------------------------------------------------------------------------------------------
    _capped("minhash_set", "ms_cut_kernel", "sketches", "ntk_minhash_set.hip", "n_rows + n_cols", 256, "kThreads", None, "0x7FFFFFFFu", None,
            "not capped by the device: one thread per sketch of a block of at most 2^26 sketches, never a second step"),
    # ---- record_minhash ------------------------------------------------------------------------------------------------------------------
    _capped("record_minhash", "rmh_windows_kernel", "records of a chunk", "ntk_record_minhash.hip", "w.r1 - w.r0", 1, "1", 8, "resident",
            ("test_gpu_record_minhash.py", "test_twenty_thousand_short_records"),
            "2 048 records per step; 20 000 records of 150 bases: 10 steps, every record with windows.  The new test has 2 560 records, "
            "empty and sub-k ones among them: a block's `continue` comes before a record that counts",
            cap_def="const unsigned resident = (unsigned)m->n_cu * kBlocksPerCu;", also=(NEW, "test_record_minhash_records_take_a_second_step")),
    _capped("record_minhash", "rmh_filter_kernel", "tiles of 256 window ends", "ntk_record_minhash.hip", "tiles", 4, "kFilterThreads / 64", 8,
            "resident", ("test_gpu_record_minhash.py", "test_records_around_the_chunk_seam"),
            "8 192 tiles per launch before a wave takes a second one (contiguous runs, no stride); a chunk of 64 Mi is 262 144 tiles: 32 "
            "per wave, and the 4 kb record at the seam is 16 of one wave's",
            cap_def="const unsigned resident = (unsigned)m->n_cu * kBlocksPerCu;"),
    _fixed("record_minhash", "rmh_retry_kernel", "segments of 4 096 window ends of one retried record", "ntk_record_minhash.hip", 1, "1", 8,
           "resident", ("test_gpu_record_minhash.py", "test_records_around_the_chunk_seam"),
           "2 048 segments = 8 Mi window ends per step.  Only the 64 MiB filler of N of the seam test strides (16 384 segments, bottom-s "
           "retries a record without a window), and no tile of it holds a window.  A retried record with windows in its second step is "
           "8 Mi + of repetitive bases, 10.5 MB at 1.25 steps and 105 MB of scratch: not reachable at a few MB, so no new test",
           cap_def="const unsigned resident = (unsigned)m->n_cu * kBlocksPerCu;"),
    # ---- kmer_sets -----------------------------------------------------------------------------------------------------------------------
    _capped("kmer_sets", "ks_join_kernel", "tiles of 2 048 key words", "ntk_kmer_sets.hip", "g.n_tiles", 2, "kMinTilesPerBlock", 4,
            "(unsigned)h->n_cu * kBlocksPerCu", (NEW, "test_kmer_sets_every_op_takes_a_third_tile"),
            "2 048 tiles in the blocks' first two; 2.7 M + 2.6 M narrow keys, or half as many wide ones, are 2 563 tiles",
            launch=r"hipLaunchKernelGGL\(\((ks_join_kernel)<\d, MODE, BINS>\), dim3\(blocks\)"),
    _capped("kmer_sets", "ks_split_kernel", "tiles", "ntk_kmer_sets.hip", "g.n_tiles + 1", 256, "kThreads", None, "0x7FFFFFFFu", None,
            "not capped by the device: one thread per tile, never a second step",
            launch=r"hipLaunchKernelGGL\((ks_split_kernel)<\d>, dim3\(split_blocks\)"),
    _capped("kmer_sets", "ks_validate_kernel", "neighbouring pairs", "ntk_kmer_sets.hip", "n - 1", 256, "kThreads", 8, "(unsigned)h->n_cu * 8",
            (NEW, "test_kmer_sets_validate_in_the_second_step"), "524 288 pairs per step; 655 360 keys",
            launch=r"hipLaunchKernelGGL\((ks_validate_kernel)<\d>, dim3\(blocks\)"),
    # ---- dbg: one grid() for every launch ------------------------------------------------------------------------------------------------
    _dbg("dbg_dir_mark_kernel", "k-mers", _N, _DBG_PAIR), _dbg("dbg_adjacency_kernel", "k-mers", _N, _DBG_PAIR),
    _dbg("dbg_link_kernel", "states", _S, _DBG_PAIR),
    _dbg("dbg_rank_init_kernel", "states", _S), _dbg("dbg_rank_round_kernel", "states", _S), _dbg("dbg_rank_cut_kernel", "states", _S),
    _dbg("dbg_resolve_kernel", "k-mers", _N), _dbg("dbg_perm_kernel", "k-mers", _N), _dbg("dbg_rows_kernel", "k-mers", _N),
    _dbg("dbg_spell_kernel", "k-mers", _N),
    # ---- colors --------------------------------------------------------------------------------------------------------------------------
    _capped("colors", "kc_add_kernel", "keys", "ntk_colors.hip", "n", 256, "kThreads", 8, "(unsigned)h->n_cu * 8",
            (NEW, "test_colors_index_of_many_keys"), "524 288 keys per step; 655 360 keys"),
    _capped("colors", "kc_lookup_kernel", "queries", "ntk_colors.hip", "n", 256, "kThreads", 8, "(unsigned)h->n_cu * 8",
            (NEW, "test_colors_index_of_many_keys"), "524 288 queries per step; 655 360 queries"),
    _capped("colors", "kc_census_kernel", "slots", "ntk_colors.hip", "h->slots", 256, "kThreads", 2, "(unsigned)h->n_cu * 2",
            ("test_gpu_colors.py", "test_from_sets_end_to_end_on_golden_data"),
            "131 072 slots per step; the golden index has 229 235 keys under its first colour alone, so 524 288 slots: 4 steps.  The new test: 98 304 + keys need "
            "262 144 slots", also=(NEW, "test_colors_index_of_many_keys")),
    _capped("colors", "kc_wave_kernel", "records", "ntk_colors.hip", "n_records", 4, "kWaveThreads / 64", 8, "(unsigned)h->n_cu * 8",
            (NEW, "test_colors_screen_records_take_a_second_step"), "8 192 records per step; 10 240 records"),
    _fixed("colors", "kc_long_kernel", "window ends of one long record", "ntk_colors.hip", 256, "kLongThreads", 4, "(unsigned)h->n_cu * 4",
           (NEW, "test_colors_one_long_record_takes_a_second_step"), "262 144 window ends per step; one record of 327 680 valid windows"),
    _capped("colors", "kc_best_kernel", "records", "ntk_colors.hip", "n_records", 256, "kThreads", 8, "(unsigned)h->n_cu * 8",
            (NEW, "test_colors_best_of_one_window_records"), "524 288 records per step; 655 360 records of one window"),
    # ---- minimizer_list: both tile kernels run once per chunk of 64 Mi bases -------------------------------------------------------------------
    _capped("minimizer_list", "ml_select_kernel", "tiles of 1 024 window ends", "ntk_minimizer_list.hip", "tiles", 1, "1", 8, "resident",
            (ML_TESTS, "test_tile_seams_of_the_select_kernel"),
            "2 048 tiles = 2 Mi window ends per step, block b takes the tiles b, b + grid, ...; the seam batch is above two steps (sparse, "
            "aimed k-mers), the exact one 1.25 steps of random reads with a quality stream, all five fields",
            cap_def="const unsigned resident = (unsigned)m->n_cu * ML_BLOCKS_PER_CU;", also=(ML_TESTS, "test_exact_past_one_step_of_the_grid")),
    _capped("minimizer_list", "ml_scatter_kernel", "tiles of 1 024 window ends", "ntk_minimizer_list.hip", "own_tiles", 1, "1", 8, "resident",
            (ML_TESTS, "test_more_tiles_than_one_step_of_the_grid"),
            "2 048 tiles per launch before a block takes a second one (a contiguous run of `per` tiles, no stride: the record starts are "
            "walked along the run); 2.5 steps of random reads are runs of 3 tiles (a digest), the exact one 1.25 steps: runs of 2; "
            "test_record_starts_carried_along_a_blocks_tiles has 2.25 steps, runs of 3 with skipped tiles and 5 000 equal starts inside them",
            cap_def="const unsigned resident = (unsigned)m->n_cu * ML_BLOCKS_PER_CU;", also=(ML_TESTS, "test_exact_past_one_step_of_the_grid")),
)


def items_per_step(row: Row, cu: int) -> Optional[int]:
    """The items one step of the whole grid takes on a device of `cu` CUs; None where the device does not cap the grid."""
    return None if row.factor is None else row.per_block * row.factor * cu


def rows_of(kernel: str, lib: Optional[str] = None) -> Row:
    found = [r for r in ROWS if r.kernel == kernel and (lib is None or r.lib == lib)]
    assert len(found) == 1, (kernel, lib)
    return found[0]


def source(name: str) -> str:
    return open(os.path.join(L.CSRC, name)).read()
