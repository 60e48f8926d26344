"""A seeded, structured, differential fuzz of sixteen libraries in thirteen stages: the twelve k-mer libraries (count table, wide count table, HyperLogLog sketch, read
abundance, read trimmer with its batch writer, MinHash; per-record MinHash, the sketch set, k-mer set algebra narrow and wide, the de
Bruijn graph, the coloured index; the minimizer lists) and the read-mapping pipeline (seed index, chains, mappings, alignments: the
stage `map_reads`) against the host models the suite already has.  Shared by tests/test_lib_fuzz_inputs.py (CPU: the
slices are not vacuous), tests/test_gpu_lib_fuzz.py (the fixed slices) and tools/lib_fuzz.py (time-budgeted runs, replay, dump).
Importable without a GPU: torch is imported only inside the device functions.

Truth is the existing models only: `_count_helpers.oracle_values` / `oracle_items`, `test_gpu_wide_count.oracle_items`,
`_sketch_model`, `_minhash_model`, `_abundance_model`, `_trim_model`, `_record_minhash_model`, `_mhset_model`, `_kmer_sets_model`,
`_dbg_model`, `_colors_model`, `_minimizer_list_model`.  Every comparison is `array_equal` / `==`, the double columns of MinHashSet.compare included (as
tests/test_gpu_minhash_set.py compares them: the counts are small, every sum is exact in a double).

The generator (`make_case`).  Query records and a related reference set (the table's batch) are sampled from one random genome of a
few kb with substitution errors, at different and uneven coverage, plus foreign reads and exact duplicates, so that abundances
differ along a record.  Record content kinds are those of tools/gpu_fuzz.py's make_input (KINDS); record lengths come from EDGE
lengths derived from the kernels' constants (`edge_lengths(k, stage)`: the six first stages share one dict, `colors`,
`record_minhash` and `minimizer_list` add their own).  The six first stages draw exactly what they drew before the newer five were added
(tests/test_lib_fuzz_inputs.py pins a digest of each slice).

The five newer stages.  `record_minhash`: per-record sketches of the batch, of a prefix and with the quality stream on one handle, the
result as a MinHashSet whose compare blocks (at most 24 x 24, a num cut and a max_hash cut) are held to `_mhset_model.block`, and one
record sketched alone by KmerMinHash beside its own row; at k = 32 with a scaled rule the batch holds the k-mer whose hash IS the
threshold, alone and inside a long record.  `kmer_sets` / `kmer_sets_wide`: two sets extracted from tables (the query batch, the
reference set), compare, totals, every op and rule, one chained op on a result nobody read back.  `dbg`: the graph of the reference
set's k-mers (with one periodic read each of DBG_UNITS, two isolated cycles), and its unitig batch handed on, as device tensors, to a
fresh count table, ReadAbundance and RecordMinHash.  `colors`: an index built colour by colour through tables, sets and per-key masks,
the batch screened, and the trimmer's compacted device batch screened as it is.  The chains keep every buffer on the device.

The `minimizer_list` stage (the twelfth library; its stage goes last, so the eleven before it draw what they drew).  (w, order) are drawn
before the records (`draw_extra`): w from four classes (ML_W_CLASSES: 1, the powers of two, their neighbours - where a window is two
overlapping ranges of the largest power of two below w -, typical ones), order LEX or HASH; the record lengths add the windows' own edges
(k + w - 2 .. k + w: no, one, two windows; k + 2 w - 1: a run of w + 1) and records of ML_TILE - 1, ML_TILE, ML_TILE + 1 window ends.  The
checker holds all five CSR fields of one handle to `_minimizer_list_model` without and with the quality stream, on a prefix of the records,
the statistics, the result where it lies on the device, the digest to the core's windowed-minimizer reduce (canonical path, LEX), and a
second, smaller batch on the same handle.  A case's batch is 6 .. 20 tiles of random, junk-bearing, masked content: what meets a tile
boundary there is proved in tests/test_lib_fuzz_inputs.py, planted wrong rules included.

The `map_reads` stage (the thirteenth, last: the twelve before it draw what they drew).  k of MAP_KS, (w, order), a pre-step of the
bit-canonical path and one value per parameter of SeedIndex.match, AnchorChains.run, ChainMappings.run and ChainAlignments.run are drawn
before the sequences (`draw_map_extra`).  `ref_records` are one to four records of a genome with a tandem repeat, a dispersed family on
both strands, N runs and lower case; `records` are the reads (`make_map_case` lists their kinds).  `pipeline_want` computes what the four
handles of a ReadMapper hold from bytes alone, through `_minimizer_list_model`, `_seed_index_model`, `_chain_model`, `_mapping_model` and
`_align_model`; `check_map_reads` holds every field and stats word of one ReadMapper per (k, w, order), kept across cases, to it: the
whole batch, a prefix on the same handles, then the thinned chains (`thinned_input`) as plain device arrays.  Left to the tests that own
them: refusals, work_mib groups, the 4095 x 4095 segment, grid steps, stream order, 2^28 spans.

Excluded inputs (what a header rules out is not generated for that stage):
  * bytes of the pre-step's "deleted" class inside a record - needletail_amd.h, "Device batch layout: ... no bytes of the pre-step's
    'deleted' class inside a record (the packer, ntk_batch_append, removed them)": none for PRE_NONE, CR / LF for PRE_STRIP_RETURNS,
    space / tab / CR / LF for PRE_NORMALIZE*; `junk_bytes(pre)` leaves them out.  The records' own break byte is the packer's '\\n';
  * PATH_BYTES_CANONICAL with PRE_NONE / PRE_STRIP_RETURNS - needletail_amd_count.h, _abundance.h, _trim.h, _minhash.h,
    _record_minhash.h, _colors.h: "Byte-path input that was not normalised ... is NTK_ERR_UNSUPPORTED": `_count_helpers.PATH_PRES` has
    no such pair;
  * k = 33..63 on a bit path, and on the abundance and trim libraries - needletail_amd_abundance.h / _trim.h: "k = 33..63 ... is not
    served here"; the wide stages draw PATH_BYTES_CANONICAL with PRE_NORMALIZE / PRE_NORMALIZE_IUPAC only; k > 32 outside
    `kmer_sets_wide` and the two older wide stages - needletail_amd_record_minhash.h and needletail_amd_colors.h hold k = 1..32,
    needletail_amd_dbg.h odd k = 3..31;
  * PATH_BITS sets and even k for the graph - needletail_amd_dbg.h: the list holds canonical k-mers of odd k (a k-mer of even k can
    be its own reverse complement); the binding refuses both, and the `dbg` stage draws DBG_KS on DBG_PATH_PRES;
  * offsets that are not the packer's - needletail_amd_abundance.h: "d_offsets[0] = 0, d_offsets[n_records] = n_bytes, record r = the
    bytes [d_offsets[r], d_offsets[r + 1]) whose last byte is the record's break byte": offsets are always `_trim_model.offsets`, or
    what ReadTrimmer.compact_device and KmerGraph.unitig_batch wrote;
  * a foreign MinHash sketch coarser than the handle - needletail_amd_minhash.h: "The counts stay exact when the other sketch keeps
    at least what this one would: the same num or a larger one, the same scaled or a divisor of it".
The 64 Mi-base chunk seams and batches above 2^32 bytes stay with the tests that own them."""
import hashlib

import numpy as np

import needletail_amd as nt
import _abundance_model as A
import _align_model as AL
import _chain_model as CH
import _colors_model as KM
import _count_model as CM
import _dbg_model as DM
import _kmer_sets_model as KS_
import _mapping_model as MP
import _mhset_model as SM
import _minhash_model as M
import _minimizer_list_model as MM
import _record_minhash_model as RM
import _seed_index_model as SI
import _sketch_model as S
import _trim_model as T
from _count_helpers import M64, PATH_PRES, oracle_items, oracle_values, pack, quality_masked, upload

BYTES, BITS, BITS_CANON = nt.PATH_BYTES_CANONICAL, nt.PATH_BITS, nt.PATH_BITS_CANONICAL
OLD_STAGES = ("count", "count_wide", "minhash", "minhash_wide", "abundance", "trim")
NEW_STAGES = ("record_minhash", "kmer_sets", "kmer_sets_wide", "dbg", "colors", "minimizer_list")
PIPELINE_STAGES = ("map_reads",)
STAGES = OLD_STAGES + NEW_STAGES + PIPELINE_STAGES   # a stage's index seeds its cases: new stages go at the end
WIDE_STAGES = ("count_wide", "minhash_wide", "kmer_sets_wide")
KS = (1, 2, 3, 15, 16, 17, 21, 31, 32)
WIDE_KS = (33, 34, 47, 48, 49, 62, 63)
WIDE_PRES = (nt.PRE_NORMALIZE, nt.PRE_NORMALIZE_IUPAC)
KINDS = ("clean", "n_runs", "breaks", "mixed", "periodic", "genome")
KIND_WEIGHTS = (0.10, 0.20, 0.10, 0.15, 0.10, 0.35)   # what the genome covers leads: records that are cut, not dropped whole
NUMS = (1, 2, 16, 500, 1 << 20)
SCALEDS = (1, 2, 7, 1000)
BUFFERS = (64, 65, 100, 256, 4096, 0)
MIN_COUNTS_ABUNDANCE = (0, 1, 2, 3)
MIN_COUNTS_TRIM = (1, 2, 3)
MODES = (T.PREFIX, T.LONGEST)
RMH_NUMS = (1, 2, 16, 64, 500, 1 << 20)
RMH_BUFFERS = (256, 257, 4096, 0)
DBG_KS = (3, 15, 17, 21, 31)
DBG_PATH_PRES = tuple(pp for pp in PATH_PRES if pp[0] != BITS)
DBG_UNITS = (b"AACGT", b"AAACCGGTTTAG")   # no rotation of either is its own reverse complement: a periodic read of one is an isolated cycle
N_COLORS = (1, 2, 3, 8, 63, 64)
ROUTES = ("table", "set", "masks")
COMPARE_SIDE = 24                # MinHashSet.compare is held to the Python model on at most 24 x 24 pairs
RMH_EDGE_MAX = 5000              # the num-dependent record lengths of the record_minhash stage stay at or below this many windows
ML_TILE = MM.TILE                # ML_TILE of ntk_ml_rule.hpp: window ends per tile of ml_select_kernel and ml_scatter_kernel
ML_W_CLASSES = {"one": (1,), "power_of_two": (2, 16, 64, 256), "neighbour": (3, 15, 17, 63, 65, 255), "typical": (5, 11, 19)}
ML_ORDERS = (MM.LEX, MM.HASH)

# the fixed slices of the GPU suite: stage -> (seed, cases).  tests/test_lib_fuzz_inputs.py proves on the CPU that each meets its
# conditions; the counts are the smallest at which they do (seeds 100..139 were searched per stage)
SLICES = {"count": (103, 3), "count_wide": (111, 3), "minhash": (134, 8), "minhash_wide": (131, 10), "abundance": (104, 3),
          "trim": (111, 4), "record_minhash": (113, 8), "kmer_sets": (117, 3), "kmer_sets_wide": (133, 2), "dbg": (127, 4),
          "colors": (130, 4), "minimizer_list": (101, 15), "map_reads": (123, 5)}

LANE_RUN = S.LANE_RUN            # kLaneRun (ntk_wide_count.hip, ntk_sketch.hip, ntk_wide_walk.hpp): window ends per lane
LONG_PIECES_BYTES = 2048 * 16    # kLongPieces (ntk_trim.hip) 16-byte pieces: beyond it a record goes to rt_copy_long_kernel
LONG_RECORD = 65536              # kLongRecord (ntk_abundance.hip): more candidate windows go to ra_block_kernel
TABLE_CAPACITY = 1 << 17         # of the tables a session keeps: above the distinct k-mers of any reference set

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b
UNITS = (b"A", b"AT", b"GC", b"ACGT", b"AATT", b"ACGTACGTTGCA")
JUNK = b"NnRYKMSWBDHVrykm-.*\x00\x7f\x80\xff0@>+"
WHITESPACE = b" \t\r\n"
DELETED = {nt.PRE_NONE: b"", nt.PRE_STRIP_RETURNS: b"\r\n", nt.PRE_NORMALIZE: WHITESPACE, nt.PRE_NORMALIZE_IUPAC: WHITESPACE}


def rmh_want(num: int) -> int:
    return 2 * num + 16          # rmh_want of ntk_rmh_rule.hpp


def edge_lengths(k: int, stage: str = "count", num: int = 0, window: int = 0) -> dict:
    """name -> record length L, each from a constant of the kernels (w = candidate windows, L = w + k - 1).  The six first stages share
    one dict; `colors`, `record_minhash` and `minimizer_list` add what their own constants name (`num`: the bottom-s size of a
    record_minhash case; `window`: the w of a minimizer_list case, k-mers per window)."""
    e = {
        "0": 0, "1": 1,                                       # the empty record (one break byte) and the shortest one
        "k-2": max(k - 2, 0), "k-1": k - 1,                   # no window
        "k": k, "k+1": k + 1, "2k-1": 2 * k - 1, "2k": 2 * k,  # one, two, k and k + 1 windows: a break in the middle leaves none / one
    }
    for L in (15, 16, 17):        # the core's 16-base lane and the copy kernels' 16-byte piece (kCopyGroup pieces of 16 B)
        e[str(L)] = L
    for L in (63, 64, 65):        # one 64-bit plane word of rt_solid_kernel; kLaneRun / kPrime of the wide walkers
        e[str(L)] = L
    for L in (127, 128, 129):     # two plane words; two lane runs
        e[str(L)] = L
    for w in (191, 192, 193):     # kRegWindows = 64 * kRegRounds of ntk_abundance.hip: the register path and the streamed one
        e[f"w{w}"] = w + k - 1
    for w in (255, 256, 257):     # kWaveInFlight * 64 of ntk_abundance.hip, and rt_solid_kernel's tile 64 * kSolidRounds
        e[f"w{w}"] = w + k - 1
    for L in (511, 512, 513):     # 32 sixteen-bit words of the materialise face's valid plane
        e[f"L{L}"] = L
    for w in (2047, 2048, 2049):  # kGroup * kGroupRounds = 32 plane words of 64 window ends: the lane group and the whole wave
        e[f"w{w}"] = w + k - 1
    if stage == "colors":
        for w in (63, 64, 65):    # one round of a wave of ntk_colors.hip's record kernel
            e[f"w{w}"] = w + k - 1
        for w in (127, 128, 129):  # two rounds
            e[f"w{w}"] = w + k - 1
    if stage == "minimizer_list":
        # no window, one, two, and a run of window + 1 windows (more than any span)
        for name, L in (("k+w-2", k + window - 2), ("k+w-1", k + window - 1), ("k+w", k + window), ("k+2w-1", k + 2 * window - 1)):
            e[name] = max(L, 0)
        for w in (ML_TILE - 1, ML_TILE, ML_TILE + 1):   # ML_TILE of ntk_ml_rule.hpp: a tile of ml_select_kernel and ml_scatter_kernel
            e[f"T{w}"] = w + k - 1
    if stage == "record_minhash":
        for w in (4095, 4096, 4097):   # kSegment of ntk_record_minhash.hip (kTile = 256 is w255 .. w257 above)
            e[f"w{w}"] = w + k - 1
        if num:                   # the all-pass length kRmhAllPass * num and rmh_want(num) of ntk_rmh_rule.hpp
            for name, w in (("4num-1", 4 * num - 1), ("4num", 4 * num), ("4num+1", 4 * num + 1), ("want-1", rmh_want(num) - 1),
                            ("want+1", rmh_want(num) + 1)):
                if w <= RMH_EDGE_MAX:
                    e[name] = w + k - 1
    return e


LONG_CLASSES = ("long_pieces", "long_record")   # kLongPieces * 16 bytes +- 17; kLongRecord + k - 1 +- 1 bases
COLORS_LONG = "colors_long"                     # kLongRecord of ntk_colors.hip (KM.LONG_RECORD) - 1, + 0, + 1 windows
ALL_LONG_CLASSES = LONG_CLASSES + (COLORS_LONG,)


def long_classes(stage: str) -> tuple:
    """The long record classes a stage draws: the tables of kmer_sets and dbg take what `count` has covered."""
    if stage in ("kmer_sets", "kmer_sets_wide", "dbg", "minimizer_list"):   # (the minimizer list's 64 Mi seam stays with its own tests)
        return ()
    return ("long_pieces", COLORS_LONG) if stage == "colors" else LONG_CLASSES


TAU_CLASSES = ("tau_alone", "tau_inside")   # a k-mer whose hash IS the scaled threshold: a record of its own, and inside a long record
TAU_INSIDE = 800                            # bases of the long one, the k-mer in its middle: more than a 256-end tile on either side


def tau_kmer(path: int, scaled: int):
    """The 32-mer whose hash is exactly max_hash(scaled), as bases, or None where its reverse complement is the canonical strand (a
    canonical path emits the other key then).  Only k = 32 spans every 64-bit key."""
    key = int(CM.fmix64_inv(np.uint64(M.max_hash(scaled)))) ^ S.XOR   # `_sketch_model.hash_keys` is fmix64(key ^ XOR)
    text = "".join("ACGT"[(key >> (2 * (31 - j))) & 3] for j in range(32))
    if path != BITS and DM.rc(text) < text:
        return None
    return text.encode()


def junk_bytes(pre: int) -> np.ndarray:
    """Non-base bytes a record may hold under `pre`: everything of gpu_fuzz's JUNK and the whitespace the pre-step does not delete."""
    ws = bytes(b for b in WHITESPACE if b not in DELETED[pre])
    return np.frombuffer(JUNK + ws, dtype=np.uint8)


class Case:
    """records / quals / qbreaks (the quality byte under each record's break byte) / cutoff: the query batch.  ref_records: the batch
    the table counts.  kinds / classes / starts: per record, its content kind, its edge-length class (None: a random length) and
    its first byte's offset in the packed batch."""

    def __init__(self, k, path, pre, stage="count", extra=None):
        self.k, self.path, self.pre, self.stage, self.extra = k, path, pre, stage, extra or {}
        self.records, self.quals, self.qbreaks, self.kinds, self.classes = [], [], [], [], []
        self.cutoff, self.ref_records = 0, []

    # packed forms ------------------------------------------------------------------------------------------------------------------
    def buf(self) -> bytes:
        return pack(self.records)

    def offsets(self) -> np.ndarray:
        return T.offsets(self.records)

    def qual_stream(self) -> np.ndarray:
        return stream(self.quals, self.qbreaks)

    def starts(self) -> np.ndarray:
        return self.offsets()[:-1].astype(np.int64)

    def num(self) -> int:
        return self.extra.get("kind", {}).get("num", 0)

    def edges(self) -> dict:
        return edge_lengths(self.k, self.stage, self.num(), self.extra.get("w", 0))

    def tag(self) -> str:
        return f"k {self.k} path {self.path} pre {self.pre} cutoff {self.cutoff} records {len(self.records)} bytes {len(self.buf())}"


def stream(quals, qbreaks) -> np.ndarray:
    """The parallel stream of a packed batch: each record's bytes, then the byte under its break byte."""
    if not quals:
        return np.zeros(0, dtype=np.uint8)
    return np.concatenate([np.append(np.frombuffer(bytes(q), dtype=np.uint8), np.uint8(b)) for q, b in zip(quals, qbreaks)]).astype(np.uint8)


def _genome_read(rng, genome, L, err=0.01):
    n = len(genome)
    if L <= n:
        s = min(int(rng.random() ** 2 * (n - L + 1)), n - L)   # uneven coverage: the genome's head is sampled more often
        r = genome[s:s + L].copy()
    else:
        r = np.resize(np.roll(genome, -int(rng.integers(0, n))), L).copy()
    sub = rng.random(L) < err
    r[sub] = ACGT[rng.integers(0, 4, int(sub.sum()))]
    if rng.random() < 0.3:
        r = COMP[r[::-1]]
    return r


def _content(rng, kind, L, k, pre, genome, at0, wide):
    """One record of `kind` and length L whose first byte lies at batch offset at0."""
    if L == 0:
        return np.zeros(0, dtype=np.uint8)
    if kind == "clean":
        return ACGT[rng.integers(0, 4, L)].copy()
    if kind == "periodic":
        a = np.resize(np.frombuffer(UNITS[int(rng.integers(0, len(UNITS)))], dtype=np.uint8), L).copy()
        for _ in range(int(rng.integers(0, 4))):
            a[int(rng.integers(0, L))] = ACGT[int(rng.integers(0, 4))]
        return a
    a = _genome_read(rng, genome, L)
    junk = junk_bytes(pre)
    if kind == "n_runs":       # runs of N of length k - 3 .. k + 3, at random places and at multiples of 16 and 64 +- 1 of the batch
        for _ in range(int(rng.integers(1, 2 + L // 150))):
            ln = max(1, k + int(rng.integers(-3, 4)))
            at = int(rng.integers(0, L))
            u = rng.random()
            if u < 0.35:
                at = (at0 + at) // 16 * 16 + int(rng.integers(-1, 2)) - at0
            elif u < 0.7:
                at = (at0 + at) // 64 * 64 + int(rng.integers(-1, 2)) - at0
            at = min(max(at, 0), L - 1)
            a[at:at + ln] = ord("N")
    elif kind == "breaks":     # a single break every k - 1 / k / k + 1 bases: no, one or two windows between breaks
        step = max(1, k + int(rng.integers(-1, 2)))
        a[step - 1::step + 1] = junk[int(rng.integers(0, junk.size))] if rng.random() < 0.5 else ord("N")
    elif kind == "mixed":      # lower case, U / u, IUPAC, whitespace the pre-step keeps, the junk bytes
        m = rng.random(L)
        a[m < 0.15] |= 0x20
        sel = m > 0.96
        a[sel] = junk[rng.integers(0, junk.size, int(sel.sum()))]
        us = (m > 0.94) & (m <= 0.96)
        a[us] = np.frombuffer(b"Uu", dtype=np.uint8)[rng.integers(0, 2, int(us.sum()))]
    if wide and kind != "genome" and rng.random() < 0.5:
        # k = 33..63: one more break within k - 1 bytes after a lane-run boundary of the batch, or one byte before it
        b = (at0 + int(rng.integers(0, L))) // LANE_RUN * LANE_RUN + int(rng.integers(-1, k)) - at0
        if 0 <= b < L:
            a[b] = ord("N")
    return a


def _qualities(rng, L, cutoff, rate):
    """Most bytes at the cutoff, a share `rate` one below it (masked: the compare is <), a tenth one above."""
    c = cutoff if cutoff else 40
    u = rng.random(L)
    q = np.full(L, c, dtype=np.uint8)
    q[u < rate] = c - 1
    q[u > 0.9] = c + 1
    return q


def make_case(rng, k, path, pre, budget=None, allow_long=True, stage="count", extra=None) -> Case:
    """One case for (k, path, pre).  See the module docstring."""
    wide = k > 32
    c = Case(k, path, pre, stage, extra)
    c.cutoff = 0 if rng.random() < 0.15 else int(rng.integers(33, 76))
    rate = float(rng.choice([0.002, 0.01, 0.05]))
    genome = ACGT[rng.integers(0, 4, int(rng.integers(2000, 4001)))]
    edges = c.edges()
    names = list(edges)
    budget = int(rng.integers(6000, 20001)) if budget is None else budget
    plan = []   # (class, L)
    longs = long_classes(stage) if allow_long else ()
    if "long_pieces" in longs and rng.random() < 0.3:
        plan.append(("long_pieces", LONG_PIECES_BYTES + int(rng.integers(-17, 18))))
    if "long_record" in longs and rng.random() < 0.12:
        plan.append(("long_record", LONG_RECORD + k - 1 + int(rng.integers(-1, 2))))
    if COLORS_LONG in longs and rng.random() < 0.5:
        plan.append((COLORS_LONG, KM.LONG_RECORD + k - 1 + int(rng.integers(-1, 2))))
    kind_ = c.extra.get("kind", {})
    tau = tau_kmer(path, kind_["scaled"]) if stage == "record_minhash" and k == 32 and "scaled" in kind_ else None
    if tau is not None:
        plan += [("tau_alone", 32), ("tau_inside", TAU_INSIDE)]
    used = 0
    while used < budget:
        if rng.random() < 0.6:
            name = names[int(rng.integers(0, len(names)))]
            plan.append((name, edges[name]))
        else:
            plan.append((None, int(rng.integers(0, 400))))
        used += plan[-1][1] + 1
    order = rng.permutation(len(plan))
    at = 0
    for i in order:
        cls, L = plan[i]
        if rng.random() < 0.25:
            # a spacer record of N that puts the next record's first byte where a kernel's geometry changes: around a lane-run
            # boundary (k = 33..63: 64m - 1 .. 64m + k - 1), or on a drawn residue of the 16-byte copy piece
            target = int(rng.integers(-1, k)) % LANE_RUN if wide else int(rng.integers(0, 16))
            pad = (target - at - 1) % (LANE_RUN if wide else 16)
            _append(c, rng, np.full(pad, ord("N"), dtype=np.uint8), "spacer", None, rate)
            at += pad + 1
        kind = KINDS[int(rng.choice(len(KINDS), p=KIND_WEIGHTS))]
        if cls in ALL_LONG_CLASSES and kind in ("clean", "periodic"):
            kind = "genome"   # a long record of foreign or one-key content says nothing about abundance and costs a hot key
        content = _content(rng, kind, L, k, pre, genome, at, wide)
        if cls in TAU_CLASSES:   # the planted k-mer alone, or in the middle of a read of the genome
            kind = "genome"
            content = _genome_read(rng, genome, L, err=0.0)
            content[(L - 32) // 2:(L - 32) // 2 + 32] = np.frombuffer(tau, dtype=np.uint8)
        _append(c, rng, content, kind, cls, rate)
        at += L + 1
    # the reference set: other reads of the same genome at another coverage, a few foreign reads, exact duplicates of query records,
    # a periodic read per unit now and then (hot keys the table holds), and T^40 at k = 32 (the key the table keeps in a side word)
    for _ in range(int(rng.integers(40, 200))):
        c.ref_records.append(_genome_read(rng, genome, int(rng.integers(50, 251))).tobytes())
    for _ in range(3):
        c.ref_records.append(ACGT[rng.integers(0, 4, int(rng.integers(40, 200)))].tobytes())
    short = [r for r in c.records if len(r) <= 600]
    for _ in range(min(3, len(short))):
        c.ref_records.append(short[int(rng.integers(0, len(short)))])
    for unit in UNITS:
        if rng.random() < 0.5:
            c.ref_records.append(bytes(np.resize(np.frombuffer(unit, dtype=np.uint8), 2 * k + int(rng.integers(0, 30)))))
    if k == 32 and rng.random() < 0.5:
        c.ref_records.append(b"T" * 40)
    if stage == "dbg":   # the graph's input alone: a periodic read per unit of DBG_UNITS, each a cycle of its own
        for unit in DBG_UNITS:
            c.ref_records.append(bytes(np.resize(np.frombuffer(unit, dtype=np.uint8), 2 * k + len(unit) + int(rng.integers(0, 30)))))
    return c


def _append(c, rng, a, kind, cls, rate):
    c.records.append(a.tobytes())
    c.quals.append(_qualities(rng, len(a), c.cutoff, rate))
    c.qbreaks.append(int(rng.integers(0, 256)))   # the byte under a break byte is ignored, whatever it is
    c.kinds.append(kind)
    c.classes.append(cls)


def draw_params(rng, stage):
    if stage == "map_reads":   # ReadMapper lists the (w, k) minimizers of the bit-canonical path
        return int(rng.choice(MAP_KS)), BITS_CANON, int(rng.choice(MAP_PRES))
    if stage in WIDE_STAGES:
        return int(rng.choice(WIDE_KS)), BYTES, int(rng.choice(WIDE_PRES))
    if stage == "dbg":
        path, pre = DBG_PATH_PRES[int(rng.integers(0, len(DBG_PATH_PRES)))]
        return int(rng.choice(DBG_KS)), path, pre
    path, pre = PATH_PRES[int(rng.integers(0, len(PATH_PRES)))]
    return int(rng.choice(KS)), path, pre


def draw_extra(rng, stage, k=None) -> dict:
    """What a new stage fixes before its records are made: the sketch rule of a record_minhash case, whose num names edge lengths; the
    window and the order of a minimizer_list case; the window, the order, the class and every parameter of a map_reads case
    (`draw_map_extra`, which needs the case's k)."""
    if stage == "map_reads":
        return draw_map_extra(rng, k)
    if stage == "minimizer_list":
        names = list(ML_W_CLASSES)
        ws = ML_W_CLASSES[names[int(rng.integers(0, len(names)))]]
        return dict(w=int(ws[int(rng.integers(0, len(ws)))]), order=int(ML_ORDERS[int(rng.integers(0, len(ML_ORDERS)))]))
    if stage != "record_minhash":
        return {}
    kind = dict(num=int(rng.choice(RMH_NUMS))) if rng.random() < 0.5 else dict(scaled=int(rng.choice(SCALEDS)))
    return dict(kind=kind, buffer_entries=int(rng.choice(RMH_BUFFERS)))


def case_rng(seed, stage, it):
    """The generator of case `it` of a stage: a stream of its own, so that a replay of case N needs no earlier case."""
    return np.random.default_rng([int(seed), STAGES.index(stage), int(it)])


def draw_case(seed, stage, it):
    """(rng, case) of iteration `it`: the rng has made the case and goes on to the checker's own draws."""
    rng = case_rng(seed, stage, it)
    k, path, pre = draw_params(rng, stage)
    if stage in OLD_STAGES:
        return rng, make_case(rng, k, path, pre)
    if stage == "map_reads":
        return rng, make_map_case(rng, k, pre, draw_extra(rng, stage, k))
    return rng, make_case(rng, k, path, pre, stage=stage, extra=draw_extra(rng, stage))


def slice_digest(stage) -> str:
    """SHA-256 over every case of the stage's slice: packed batch, quality stream, packed reference set and parameters, each with its
    length in front."""
    h = hashlib.sha256()
    seed, n = SLICES[stage]
    for it in range(1, n + 1):
        _, c = draw_case(seed, stage, it)
        parts = (c.buf(), c.qual_stream().tobytes(), pack(c.ref_records), repr((c.k, c.path, c.pre, c.cutoff)).encode())
        if stage in PIPELINE_STAGES:   # the drawn parameters are the case as much as its bytes are
            parts += (repr(sorted(c.extra.items())).encode(),)
        for part in parts:
            h.update(len(part).to_bytes(8, "little"))
            h.update(part)
    return h.hexdigest()


# ---- the models' side -------------------------------------------------------------------------------------------------------------------

def wide_items(buf: bytes, k: int):
    from test_gpu_wide_count import oracle_items as wide_oracle_items   # (its module imports torch)
    return wide_oracle_items(buf, k)


def oracle_keys(buf: bytes, k: int, path: int, pre: int) -> np.ndarray:
    """Every key the batch emits, with repeats: narrow values, or [hi, lo] rows at k >= 33."""
    if k <= 32:
        return oracle_values(buf, k, path, pre)
    keys, counts = wide_items(buf, k)
    return np.repeat(keys, counts, axis=0)


def items_of(buf: bytes, k: int, path: int, pre: int):
    return oracle_items(buf, k, path, pre) if k <= 32 else wide_items(buf, k)


def masked_buf(case, use_q: bool) -> bytes:
    return quality_masked(case.buf(), case.qual_stream(), case.cutoff) if use_q else case.buf()


def draw_minhash(rng):
    """(kind, buffer_entries, use_q, pieces, ops, reset_after) of a MinHash case: the checker's draws, in one place for the CPU test."""
    kind = dict(num=int(rng.choice(NUMS))) if rng.random() < 0.5 else dict(scaled=int(rng.choice(SCALEDS)))
    buffer_entries = int(rng.choice(BUFFERS))
    use_q = bool(rng.random() < 0.5)
    pieces = int(rng.integers(1, 6))
    ops = [("stats", "hashes", "nothing", "merge")[int(rng.integers(0, 4))] for _ in range(pieces)]
    reset_after = int(rng.integers(0, pieces)) if rng.random() < 0.25 else -1
    return kind, buffer_entries, use_q, pieces, ops, reset_after


def draw_trim(rng, k):
    """(mode, min_count, min_length) of the setting whose rows a trim case compacts and feeds back."""
    return int(rng.choice(MODES)), int(rng.choice(MIN_COUNTS_TRIM)), int(rng.choice([0, k, 2 * k]))


def finer(rng, kind) -> dict:
    """The same rule or a finer one: a sketch that keeps at least what `kind` would (the header's condition for an exact merge)."""
    if "num" in kind:
        return dict(num=min(kind["num"] * int(rng.choice([1, 2, 5])), M.MAX_NUM))
    return dict(scaled=int(rng.choice([d for d in (1, 2, 7, 500, 1000) if kind["scaled"] % d == 0])))


def split_records(case, pieces: int):
    """The records in `pieces` runs; each run but the last is followed by empty records (single break bytes) up to the next multiple
    of 16, so that every call starts 16-byte aligned on a record boundary (test_gpu_minhash's _cuts, made to order).  Returns the
    packed buffer, the quality stream and the cut points."""
    n = len(case.records)
    bounds = sorted({n * j // pieces for j in range(1, pieces)} - {0, n})
    seq, qual, cuts = bytearray(), bytearray(), [0]
    qs = case.qual_stream().tobytes()
    off = case.offsets()
    for i in range(n):
        if i in bounds:
            pad = -len(seq) % 16
            seq += b"\n" * pad
            qual += b"\x00" * pad
            cuts.append(len(seq))
        seq += case.records[i] + b"\n"
        qual += qs[int(off[i]):int(off[i + 1])]
    cuts.append(len(seq))
    return bytes(seq), np.frombuffer(bytes(qual), dtype=np.uint8), cuts


def compacted_records(case, rows, want):
    """The model's compacted batch as records: (records, quality bytes, the bytes under the break bytes) of `_trim_model.compact`'s
    result `want` for the trimmer's `rows`."""
    src = [int(s) for s in want[3]]
    o_recs = [case.records[s][int(rows[s][0]):int(rows[s][0] + rows[s][1])] for s in src]
    o_quals = [case.quals[s][int(rows[s][0]):int(rows[s][0] + rows[s][1])] for s in src]
    return o_recs, o_quals, [case.qbreaks[s] for s in src]


def _draw_range(rng, n: int):
    """A range of at most COMPARE_SIDE of n sketches: (first, end)."""
    count = int(rng.integers(1, min(COMPARE_SIDE, n) + 1))
    first = int(rng.integers(0, n - count + 1))
    return first, first + count


def draw_rmh(rng, case) -> dict:
    """The checker's draws of a record_minhash case (its rule and buffer were drawn before the records: `draw_extra`)."""
    n = len(case.records)
    return dict(prefix=int(rng.integers(1, n + 1)), prefix_q=bool(rng.random() < 0.5), abundance=bool(rng.random() < 0.5),
                num_cut=int(rng.choice((1, 2, 16, 500, 2048, 2049))), hash_cut=float(rng.random()), rows=_draw_range(rng, n),
                cols=_draw_range(rng, n), probe=int(rng.integers(0, n)), trim=bool(rng.random() < 0.3))


def rmh_values(case, use_q: bool):
    return [RM.record_values(r, case.k, case.path, case.pre, case.quals[i] if use_q else None, case.cutoff)
            for i, r in enumerate(case.records)]


def csr_sketches(csr):
    """The (hashes, counts) pairs of a CSR of sketches."""
    off, _, h, c = csr
    return [(h[int(off[r]):int(off[r + 1])], c[int(off[r]):int(off[r + 1])]) for r in range(off.size - 1)]


def hash_cut_of(sketches, u: float) -> int:
    """The max_hash cut of a compare: the hash at quantile u of the compared rows' hashes, so that it cuts inside them."""
    pool = np.concatenate([h for h, _ in sketches]) if sketches else np.zeros(0, dtype=np.uint64)
    return int(np.sort(pool)[int(u * pool.size)]) if pool.size else M.ALL // 2


RULE_NAMES = {KS_.MIN: "min", KS_.MAX: "max", KS_.SUM: "sum", KS_.LEFT: "left", KS_.RIGHT: "right"}


def draw_ksets(rng) -> dict:
    ops = [KS_.OPS[int(rng.integers(0, len(KS_.OPS)))] for _ in range(2)]
    return dict(mc_a=int(rng.integers(1, 4)), mc_b=int(rng.integers(1, 4)), bins=(int(rng.integers(2, 33)), int(rng.integers(2, 9))),
                ops=ops, left=bool(rng.random() < 0.5), release=bool(rng.random() < 0.3))


def ksets_operands(case, d):
    """The two operands as the model's dicts: the query batch's items and the reference set's, each from its min_count on."""
    out = []
    for buf, mc in ((case.buf(), d["mc_a"]), (pack(case.ref_records), d["mc_b"])):
        keys, counts = items_of(buf, case.k, case.path, case.pre)
        keep = counts >= mc
        out.append(KS_.as_dict(keys[keep], counts[keep]))
    return out


def ksets_chain(d, da, db):
    """The chained step on the model: the result of the first drawn op is an operand of the second."""
    (op1, rule1), (op2, rule2) = d["ops"]
    first = KS_.apply(op1, rule1, da, db)
    return KS_.apply(op2, rule2, first, db) if d["left"] else KS_.apply(op2, rule2, da, first)


def draw_dbg(rng) -> dict:
    return dict(min_count=int(rng.choice((1, 2))), release=bool(rng.random() < 0.3))


def dbg_graph(case, d):
    """(keys, counts, the model's graph) of the reference set's items with count >= min_count."""
    keys, counts = oracle_items(pack(case.ref_records), case.k, case.path, case.pre)
    keep = counts >= d["min_count"]
    return keys[keep], counts[keep].astype(np.uint64), DM.Graph(keys[keep], counts[keep], case.k)


def random_masks(rng, n, n_colors):
    """Masks with no bit, one bit, several, all bits of the index, the last colour's bit, and (below 64 colours) bits beyond it."""
    bits = KM.color_bits(n_colors)
    kind = rng.integers(0, 6, n)
    one = np.uint64(1) << rng.integers(0, n_colors, n).astype(np.uint64)
    some = (rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64))
    m = np.select([kind == 0, kind == 1, kind == 2, kind == 3, kind == 4],
                  [np.zeros(n, np.uint64), one, some & np.uint64(bits), np.full(n, bits, np.uint64), np.full(n, 1 << (n_colors - 1), np.uint64)],
                  some)   # kind 5: as drawn, bits at or above n_colors among them
    return m.astype(np.uint64)


def draw_colors(rng, case) -> dict:
    """The checker's draws of a colors case.  groups[c]: the reference records of colour c (record i goes to colour i mod n_colors, and
    to every other colour with probability min(1 / 2, 1 / n_colors)); routes[c] of ROUTES; star: a colour added through a table whose
    hits are held to ReadAbundance (None: no table route); dead: a query record of foreign content whose k-mers are added with bits at
    or above n_colors only (None: 64 colours, or no such record)."""
    n_colors = int(rng.choice(N_COLORS))
    nref = len(case.ref_records)
    member = rng.random((nref, n_colors)) < min(0.5, 1.0 / n_colors)
    member[np.arange(nref), np.arange(nref) % n_colors] = True
    routes = [ROUTES[int(rng.integers(0, 3))] for _ in range(n_colors)]
    tables = [c for c in range(n_colors) if routes[c] == "table"]
    foreign = [i for i, (r, kind) in enumerate(zip(case.records, case.kinds)) if kind == "clean" and len(r) >= case.k]
    n = len(case.records)
    return dict(n_colors=n_colors, groups=[np.flatnonzero(member[:, c]).tolist() for c in range(n_colors)], routes=routes,
                min_counts=[int(rng.integers(1, 3)) for _ in range(n_colors)], mask_seeds=[int(rng.integers(0, 1 << 31)) for _ in range(n_colors)],
                star=tables[int(rng.integers(0, len(tables)))] if tables else None,
                dead=foreign[int(rng.integers(0, len(foreign)))] if foreign and n_colors < KM.COLORS_MAX else None,
                dead_bit=int(rng.integers(n_colors, KM.COLORS_MAX)) if n_colors < KM.COLORS_MAX else None,
                prefix=int(rng.integers(1, n + 1)), prefix_q=bool(rng.random() < 0.5), trim=draw_trim(rng, case.k))


def colors_steps(case, d):
    """(model, steps): the index as `_colors_model.Index` and what the device is to add, in order: ("table" | "set", colour, min_count,
    packed group) for the list routes first, then ("masks", colour, None, (keys, masks)) for the mask routes and the dead keys.  A colour
    whose group has no k-mer adds nothing."""
    k, path, pre = case.k, case.path, case.pre
    model, lists, masks = KM.Index(d["n_colors"]), [], []
    for c in range(d["n_colors"]):
        buf = pack([case.ref_records[i] for i in d["groups"][c]])
        keys, counts = oracle_items(buf, k, path, pre)
        route, mc = d["routes"][c], d["min_counts"][c]
        if route == "masks":
            if keys.size:
                m = random_masks(np.random.default_rng(d["mask_seeds"][c]), keys.size, d["n_colors"])
                masks.append(("masks", c, None, (keys, m)))
        elif (counts >= mc).any():
            lists.append((route, c, mc, buf))
            model.add(keys[counts >= mc], 1 << c)
    if d["dead"] is not None:
        keys = np.unique(KM.record_values(case.records[d["dead"]], k, path, pre))
        if keys.size:
            masks.append(("masks", None, None, (keys, np.full(keys.size, 1 << d["dead_bit"], dtype=np.uint64))))
    for _, _, _, (keys, m) in masks:
        model.add(keys, m)
    return model, lists + masks


def colors_values(case, use_q: bool):
    return [KM.record_values(r, case.k, case.path, case.pre, case.quals[i] if use_q else None, case.cutoff) for i, r in enumerate(case.records)]


def draw_ml(rng, case) -> dict:
    """The checker's draws of a minimizer_list case (its window and order were drawn before the records: `draw_extra`)."""
    n = len(case.records)
    return dict(prefix=int(rng.integers(1, n + 1)), prefix_q=bool(rng.random() < 0.5), second_q=bool(rng.random() < 0.5),
                second_budget=int(rng.integers(200, 3000)), trim=bool(rng.random() < 0.3))


def ml_entries(case, use_q: bool, n_records=None):
    """(the model's entries, offsets, n_bytes) of the case's first `n_records` records (None: all): the packed buffer cut at that
    record's end, `_trim_model.offsets`, and the quality stream where `use_q`."""
    off = case.offsets()
    m = len(case.records) if n_records is None else n_records
    n_bytes = int(off[m])
    qual = case.qual_stream()[:n_bytes] if use_q else None
    ent = MM.entries_of(case.buf()[:n_bytes], case.k, case.extra["w"], case.path, case.pre, case.extra["order"], qual, case.cutoff)
    return ent, off[:m + 1], n_bytes


def ml_want(case, use_q: bool, n_records=None):
    """The CSR `MinimizerList.read()` is held to."""
    ent, off, n_bytes = ml_entries(case, use_q, n_records)
    return MM.csr(ent, off, n_bytes, case.k)


def ml_second_case(rng, case, d) -> Case:
    """The second, smaller batch of a minimizer_list case: the same parameters, window and order."""
    return make_case(rng, case.k, case.path, case.pre, budget=d["second_budget"], allow_long=False, stage=case.stage, extra=case.extra)


def trim_chain(case, items, setting):
    """(rows, compact) of the model for the setting a chain compacts, with the quality mask: `_trim_model.rows` and `.compact`."""
    mode, mc, ml = setting
    rows = T.rows(case.records, items, case.k, case.path, case.pre, mode, mc, ml, case.quals, case.cutoff)
    return rows, T.compact(case.records, rows, case.quals, case.qbreaks)


# ---- the device side --------------------------------------------------------------------------------------------------------------------

class Session:
    """What outlives a case: the context, and per (k, path) one table with its abundance and trim handles, whose scratch grows and
    shrinks from case to case; likewise one handle per (stage, k, path, ...) of the newer libraries (`handle`)."""

    def __init__(self, ctx):
        self.ctx, self.handles, self.others = ctx, {}, {}

    def table(self, k, path):
        if (k, path) not in self.handles:
            t = nt.KmerTable(k, path, TABLE_CAPACITY, self.ctx)
            self.handles[(k, path)] = (t, nt.ReadAbundance(t), nt.ReadTrimmer(t))
        return self.handles[(k, path)]

    def counted(self, case):
        """The session's table of (k, path) after it counted the case's reference set, its handles, and the oracle's items."""
        t, ra, rt = self.table(case.k, case.path)
        buf = pack(case.ref_records)
        t.reset()
        t.count_device(upload(buf), len(buf), case.pre)
        self.ctx.synchronize()
        return t, ra, rt, oracle_items(buf, case.k, case.path, case.pre)

    def handle(self, key, make):
        """The handle kept under `key` (a tuple that begins with what it is for), made by `make()` on first use."""
        if key not in self.others:
            self.others[key] = make()
        return self.others[key]

    def rmh(self, stage, k, path, kind, buffer_entries):
        return self.handle((stage, "rmh", k, path, tuple(kind.items()), buffer_entries),
                           lambda: nt.RecordMinHash(k, path, ctx=self.ctx, buffer_entries=buffer_entries, **kind))

    def scratch_table(self, stage, k, path):
        """A second table of (k, path): what a stage counts besides the reference set (narrow or wide by k)."""
        cls = nt.KmerTable if k <= 32 else nt.WideKmerTable
        return self.handle((stage, "table", k, path), lambda: cls(k, path, TABLE_CAPACITY, self.ctx))

    def close(self):
        for h in self.others.values():
            h.close()
        for t, ra, rt in self.handles.values():
            rt.close(); ra.close(); t.close()
        self.handles, self.others = {}, {}


class Mismatch(AssertionError):
    pass


def _eq(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or not np.array_equal(got, want):
        where = ""
        if got.shape == want.shape and got.size:
            bad = np.argwhere(got != want)[0].tolist()
            where = f"; first at {bad}: got {got[tuple(bad)]}, want {want[tuple(bad)]}"
        raise Mismatch(f"{what}: shapes {got.shape} / {want.shape}{where}")


def _dev_u64(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _host(t) -> np.ndarray:
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def check_count(sess, case, rng):
    """KmerSketch registers and n_windows, then items, stats, spectrum and lookups of the table the sketch sizes."""
    k, path, pre = case.k, case.path, case.pre
    buf = case.buf()
    fill = ord("A") if rng.random() < 0.5 else ord("\n")   # readable padding of bases past n_bytes is not input
    dev, dq = upload(buf, fill=fill), upload(case.qual_stream().tobytes(), fill=0xFF)
    ref_keys = items_of(pack(case.ref_records), k, path, pre)[0]
    for use_q in (False, True):
        what = f"count quality {use_q}"
        kw = dict(d_qual=dq, quality_cutoff=case.cutoff) if use_q else {}
        keys = oracle_keys(masked_buf(case, use_q), k, path, pre)
        want = np.unique(keys, axis=0, return_counts=True) if keys.shape[0] else (keys, np.zeros(0, dtype=np.int64))
        with nt.KmerSketch(k, path, sess.ctx) as sk:
            sk.add_device(dev, len(buf), pre, **kw)
            _eq(sk.registers(), S.registers(keys), what + " registers")
            _eq(sk.estimate()["n_windows"], keys.shape[0], what + " n_windows")
            with sk.table() as t:
                t.count_device(dev, len(buf), pre, **kw)
                got = t.items()
                _eq(got[0], want[0], what + " keys")
                _eq(got[1], want[1].astype(np.uint64), what + " counts")
                st = t.stats()
                _eq([st["n_distinct"], st["n_total"], st["n_dropped"]], [len(want[0]), int(want[1].sum()), 0], what + " stats")
                _eq(t.spectrum(64), np.bincount(np.minimum(want[1], 63), minlength=64).astype(np.uint64), what + " spectrum")
                # present keys, keys of the reference set (present or absent), and the all-T key
                q = np.concatenate([want[0][::3], ref_keys[: 4000]])
                if k == 32 and path == BITS:
                    q = np.concatenate([q, np.array([M64], dtype=np.uint64)])
                if q.shape[0]:
                    _eq(t.lookup(q), _lookup(q, want), what + " lookup")


def _lookup(q, items):
    """Counts of the queried keys in the oracle's items (absent = 0): `_abundance_model.lookup`, on [hi, lo] rows through a dict."""
    if q.ndim == 1:
        return A.lookup(q, (items[0], items[1].astype(np.uint64)))
    d = {(int(h), int(lo)): int(c) for (h, lo), c in zip(items[0], items[1])}
    return np.array([d.get((int(h), int(lo)), 0) for h, lo in q], dtype=np.uint64)


def _assert_minhash(mh, keys, kind, first, what):
    want = M.sketch(keys, **kind)
    if first == "stats":
        st, (h, c) = mh.stats(), mh.hashes()
    else:
        (h, c), st = mh.hashes(), mh.stats()
    _eq(h, want[0], what + " hashes")
    _eq(c, want[1], what + " counts")
    _eq([st["n_windows"], st["n_kept"], st["threshold"]], [keys.shape[0], want[0].size, M.threshold(want[0], **kind)], what + " stats")


def check_minhash(sess, case, rng):
    """One handle through 1..5 add_device calls with stats / hashes / nothing / merge between them, now and then a reset."""
    k, path, pre = case.k, case.path, case.pre
    kind, buffer_entries, use_q, pieces, ops, reset_after = draw_minhash(rng)
    other = make_case(rng, k, path, pre, budget=int(rng.integers(200, 3000)), allow_long=False)
    what = f"minhash {kind} buffer {buffer_entries} quality {use_q} pieces {pieces} ops {ops} reset_after {reset_after}"
    buf, qual, cuts = split_records(case, pieces)
    dev, dq = upload(buf, fill=ord("A")), upload(qual.tobytes(), fill=0xFF)
    masked = quality_masked(buf, qual, case.cutoff) if use_q else buf
    empty = np.zeros((0,) if k <= 32 else (0, 2), dtype=np.uint64)
    with nt.KmerMinHash(k, path, ctx=sess.ctx, buffer_entries=buffer_entries, **kind) as mh:
        keys = [empty]
        i = 0
        while i < len(cuts) - 1:
            a, b = cuts[i], cuts[i + 1]
            kw = dict(d_qual=dq.data_ptr() + a, quality_cutoff=case.cutoff) if use_q else {}
            mh.add_device(dev.data_ptr() + a, b - a, pre, **kw)
            keys.append(oracle_keys(masked[a:b], k, path, pre))
            op = ops[i]
            if op == "merge":
                okind = finer(rng, kind)
                obuf = other.buf()
                okeys = oracle_keys(obuf, k, path, pre)
                with nt.KmerMinHash(k, path, ctx=sess.ctx, buffer_entries=int(rng.choice(BUFFERS)), **okind) as mo:
                    mo.add_device(upload(obuf), len(obuf), pre)
                    _assert_minhash(mo, okeys, okind, "hashes", what + f" other {okind}")
                    if rng.random() < 0.5:
                        mh.merge(mo)
                    else:
                        h, c = mo.hashes()
                        mh.merge(h, c, n_windows=okeys.shape[0])
                keys.append(okeys)
            if op != "nothing":
                _assert_minhash(mh, np.concatenate(keys), kind, "stats" if op == "stats" else "hashes", what + f" after piece {i} {op}")
            if i == reset_after:
                mh.reset()
                keys, reset_after, i = [empty], -1, 0   # start over: the handle is as new
                continue
            i += 1
        _assert_minhash(mh, np.concatenate(keys), kind, "hashes", what + " at the end")
    return what


def check_abundance(sess, case, rng):
    """Rows for min_count 0..3 with and without the quality stream, then a shorter batch and the whole one again on the same handle."""
    k, path, pre = case.k, case.path, case.pre
    t, ra, rt, items = sess.counted(case)
    buf, off = case.buf(), case.offsets()
    n = len(case.records)
    dev, dq, d_off = upload(buf), upload(case.qual_stream().tobytes(), fill=0xFF), _dev_u64(off)
    for use_q in (False, True):
        kw = dict(d_qual=dq, quality_cutoff=case.cutoff) if use_q else {}
        values = [A.record_values(r, k, path, pre, case.quals[i] if use_q else None, case.cutoff) for i, r in enumerate(case.records)]
        for mc in MIN_COUNTS_ABUNDANCE:
            want = A.rows_from_values(values, items, mc)
            _eq(_host(ra.run_device(dev, len(buf), d_off, n, pre, min_count=mc, **kw)), want, f"abundance quality {use_q} min_count {mc}")
        m = int(rng.integers(0, n + 1))   # a prefix of the batch: the scratch shrinks; the bytes after it are readable and not input
        if m:
            got = _host(ra.run_device(dev, int(off[m]), d_off, m, pre, min_count=2, **kw))
            _eq(got, A.rows_from_values(values[:m], items, 2), f"abundance quality {use_q} first {m} records")
    if rng.random() < 0.3:
        ra.trim()


def check_trim(sess, case, rng):
    """Rows of both modes, the compaction with the quality bytes as the parallel stream, and the compacted device tensors handed
    unchanged to a fresh count table, the abundance call and the trimmer again."""
    k, path, pre, cutoff = case.k, case.path, case.pre, case.cutoff
    t, ra, rt, items = sess.counted(case)
    recs, buf, off = case.records, case.buf(), case.offsets()
    n = len(recs)
    qs = case.qual_stream()
    dev, dq, d_off = upload(buf), upload(qs.tobytes(), fill=0xFF), _dev_u64(off)
    for use_q in (False, True):
        kw = dict(d_qual=dq, quality_cutoff=cutoff) if use_q else {}
        wins = [T.record_windows(r, k, path, pre, case.quals[i] if use_q else None, cutoff) for i, r in enumerate(recs)]
        for mode in MODES:
            for mc in MIN_COUNTS_TRIM:
                for ml in (0, k, 2 * k):
                    want = T.rows_from_windows(recs, wins, items, k, mode, mc, ml)
                    got = rt.run_device(dev, len(buf), d_off, n, pre, min_count=mc, mode=mode, min_length=ml, **kw)
                    _eq(_host(got), want, f"trim quality {use_q} mode {mode} min_count {mc} min_length {ml}")
    # the compaction of one drawn setting (rows with the quality mask, whose windows are still in `wins`)
    mode, mc, ml = draw_trim(rng, k)
    what = f"trim round trip mode {mode} min_count {mc} min_length {ml}"
    want_rows = T.rows_from_windows(recs, wins, items, k, mode, mc, ml)
    d_rows = rt.run_device(dev, len(buf), d_off, n, pre, min_count=mc, mode=mode, min_length=ml, d_qual=dq, quality_cutoff=cutoff)
    want = T.compact(recs, want_rows, case.quals, case.qbreaks)
    out = rt.compact_device(dev, len(buf), d_off, n, d_rows, dq)
    pad = len(want[0])
    _eq(out[1], want[1], what + " n_bytes")
    _eq(_host(out[0])[:pad], np.frombuffer(want[0], dtype=np.uint8), what + " bytes and padding")
    _eq(_host(out[2]), want[2], what + " offsets")
    _eq(_host(out[3]), want[3], what + " sources")
    _eq(_host(out[4])[:pad], np.frombuffer(want[4], dtype=np.uint8), what + " aux bytes and padding")
    n_out = len(want[3])
    if n_out == 0:
        return what
    # the model's compacted records; the device tensors go on as they are
    o_recs, o_quals, o_breaks = compacted_records(case, want_rows, want)
    o_buf, o_qs = pack(o_recs), stream(o_quals, o_breaks)
    assert o_buf == want[0][:want[1]]
    with nt.KmerTable(k, path, max(want[1], 16), sess.ctx) as fresh:
        fresh.count_device(out[0], out[1], pre, d_qual=out[4], quality_cutoff=cutoff)
        w = oracle_items(quality_masked(o_buf, o_qs, cutoff), k, path, pre)
        got = fresh.items()
        _eq(got[0], w[0], what + " recount keys")
        _eq(got[1], w[1].astype(np.uint64), what + " recount counts")
    _eq(_host(ra.run_device(out[0], out[1], out[2], n_out, pre, d_qual=out[4], quality_cutoff=cutoff, min_count=mc)),
        A.rows(o_recs, items, k, path, pre, mc, o_quals, cutoff), what + " abundance of the output")
    _eq(_host(rt.run_device(out[0], out[1], out[2], n_out, pre, d_qual=out[4], quality_cutoff=cutoff, min_count=mc, mode=mode, min_length=ml)),
        T.rows(o_recs, items, k, path, pre, mode, mc, ml, o_quals, cutoff), what + " trim of the output")
    if rng.random() < 0.3:
        rt.release()
    return what


def _eq_csr(got, want, what):
    for name, g, w in zip(("offsets", "n_windows", "hashes", "counts"), got, want):
        _eq(g, w, f"{what} {name}")


def _eq_block(got, want, what):
    """A compare block as tests/test_gpu_minhash_set.py's assert_block holds it: integers, vectors and doubles with array_equal."""
    for name in SM.MATRICES + ("n_a", "n_b"):
        if got[name].dtype != want[name].dtype:
            raise Mismatch(f"{what} {name}: dtype {got[name].dtype} / {want[name].dtype}")
        _eq(got[name], want[name], f"{what} {name}")


def check_record_minhash(sess, case, rng):
    """Per-record sketches of the batch without the quality stream, of a prefix, and with it, on one handle; then the last result as a
    sketch set whose compare blocks are held to the model, and one record sketched alone by KmerMinHash beside its own row."""
    k, path, pre, cutoff = case.k, case.path, case.pre, case.cutoff
    kind, buffer_entries = case.extra["kind"], case.extra["buffer_entries"]
    d = draw_rmh(rng, case)
    what = f"record_minhash {kind} buffer {buffer_entries} {d}"
    buf, off, n = case.buf(), case.offsets(), len(case.records)
    dev, dq, d_off = upload(buf, fill=ord("A")), upload(case.qual_stream().tobytes(), fill=0xFF), _dev_u64(off)
    rmh = sess.rmh(case.stage, k, path, kind, buffer_entries)
    values = {False: rmh_values(case, False), True: rmh_values(case, True)}
    q = dict(d_qual=dq, quality_cutoff=cutoff)
    rmh.run_device(dev, len(buf), d_off, n, pre)
    _eq_csr(rmh.sketches(), RM.csr(values[False], **kind), what + " whole batch")
    m = d["prefix"]   # the bytes after the prefix are readable and are not input
    rmh.run_device(dev, int(off[m]), d_off, m, pre, **(q if d["prefix_q"] else {}))
    _eq_csr(rmh.sketches(), RM.csr(values[d["prefix_q"]][:m], **kind), what + f" first {m} records")
    rmh.run_device(dev, len(buf), d_off, n, pre, **q)
    want = RM.csr(values[True], **kind)
    _eq_csr(rmh.sketches(), want, what + " whole batch with qualities")
    # the set behind it
    sk = csr_sketches(want)
    s = sess.handle((case.stage, "mhset", d["abundance"]), lambda: nt.MinHashSet(d["abundance"], sess.ctx))
    s.reset()
    _eq(list(s.add_record_sketches(rmh)), list(range(n)), what + " indices of the set")
    (r0, r1), (c0, c1) = d["rows"], d["cols"]
    for num, max_hash in ((d["num_cut"], M.ALL), (0, hash_cut_of(sk[r0:r1], d["hash_cut"]))):
        got = s.compare(rows=(r0, r1), cols=(c0, c1), num=num, max_hash=max_hash)
        _eq_block(got, SM.block(sk[r0:r1], sk[c0:c1], num, max_hash, d["abundance"]), what + f" compare num {num} max_hash {max_hash}")
    # one record alone through KmerMinHash: its row is the record's own
    r = d["probe"]
    one, one_q = upload(case.records[r] + b"\n"), upload(bytes(case.quals[r]) + bytes([case.qbreaks[r]]), fill=0xFF)
    with nt.KmerMinHash(k, path, ctx=sess.ctx, **kind) as mh:
        mh.add_device(one, len(case.records[r]) + 1, pre, d_qual=one_q, quality_cutoff=cutoff)
        idx = s.add(mh)
    _eq(idx, n, what + " index of the added sketch")
    alone, own = s.compare(rows=idx, cols=(0, n)), s.compare(rows=r, cols=(0, n))
    for name in SM.MATRICES + ("n_a", "n_b"):
        _eq(alone[name], own[name], what + f" record {r} alone, {name}")
    if d["trim"]:
        rmh.trim()
    return what


def _apply_op(a, b, op, rule):
    if op == KS_.INTERSECT:
        return a.intersect(b, RULE_NAMES[rule])
    if op == KS_.UNION:
        return a.union(b, RULE_NAMES[rule])
    return a.subtract(b) if op == KS_.SUBTRACT else a.counters_subtract(b)


def _eq_set(got, want: dict, what):
    keys, counts = got.items()
    wk, wc = KS_.as_list(want, got.key_words)
    _eq(len(got), len(want), what + " length")
    _eq(keys, wk, what + " keys")
    _eq(counts, wc, what + " counts")
    _eq(got.violations(), 0, what + " violations")


def check_kmer_sets(sess, case, rng):
    """Two sets extracted from tables (the query batch's and the session table's, which counted the reference set): compare, totals,
    every op and rule, and one chained step whose middle result stays on the device."""
    k, path, pre = case.k, case.path, case.pre
    d = draw_ksets(rng)
    what = f"kmer_sets {d}"
    da, db = ksets_operands(case, d)
    buf, ref = case.buf(), pack(case.ref_records)
    ta, tb = sess.scratch_table(case.stage, k, path), sess.scratch_table(case.stage + " reference", k, path)
    devs = [upload(buf), upload(ref)]   # both stay until the context's stream has read them
    for t, b, dev in ((ta, buf, devs[0]), (tb, ref, devs[1])):
        t.reset()
        t.count_device(dev, len(b), pre)
    sess.ctx.synchronize()
    with nt.KmerSet.from_table(ta, d["mc_a"]) as a, nt.KmerSet.from_table(tb, d["mc_b"]) as b:
        _eq_set(a, da, what + " the query batch's set")
        _eq_set(b, db, what + " the reference set's set")
        hist, totals = a.compare(b, *d["bins"])
        want_hist, want_totals = KS_.compare(da, db, *d["bins"])
        _eq(hist.reshape(-1), want_hist, what + " hist")
        _eq(totals == want_totals, True, what + f" totals {totals} / {want_totals}")
        _eq(a.totals(b) == KS_.compare(da, db, 2, 2)[1], True, what + " totals of a 2 x 2 compare")
        for op, rule in KS_.OPS:
            with _apply_op(a, b, op, rule) as out:
                _eq_set(out, KS_.apply(op, rule, da, db), what + f" op {op} rule {rule}")
        (op1, rule1), (op2, rule2) = d["ops"]
        with _apply_op(a, b, op1, rule1) as first:   # not read back: the second op takes it from the device
            with (_apply_op(first, b, op2, rule2) if d["left"] else _apply_op(a, first, op2, rule2)) as second:
                _eq_set(second, ksets_chain(d, da, db), what + " chained")
        if d["release"]:
            a.release()
    return what


def hold_graph(g, m, n_keys: int, name):
    """Everything a KmerGraph answers, held to the model `m` of its list (tests/test_gpu_dbg.py's `hold`).  Returns (stats, the unitig
    batch as the graph handed it out)."""
    edges, totals = g.edges().cpu().numpy(), g.totals()
    u = g.unitigs()
    seq, n_bytes, offsets, n_records = g.unitig_batch()
    stats = g.stats()
    assert np.array_equal(edges, m.edges), name
    want = m.totals()
    for key in DM.TOTALS:
        assert np.array_equal(totals[key], want[key]), (name, key, totals[key], want[key])
    assert (u.n_unitigs, u.n_bases) == (m.n_unitigs, m.n_bases), name
    assert np.array_equal(u.kmer_rows.cpu().numpy().view(np.uint32), m.kmer_rows), name
    assert np.array_equal(u.unitig_rows.cpu().numpy().view(np.uint64), m.unitig_rows), name
    assert int(m.unitig_rows[:, 1].sum()) == n_keys
    text, off = m.batch()
    assert n_bytes == int(off[-1]) and n_records == m.n_unitigs, name
    assert np.array_equal(offsets.cpu().numpy().view(np.uint64), off), name
    assert np.array_equal(seq[: text.size].cpu().numpy(), text), name
    assert bool((seq[text.size:] == ord("\n")).all()), name
    return stats, (seq, n_bytes, offsets, n_records)


def check_dbg(sess, case, rng):
    """The graph of the reference set's k-mers from a min_count on, and its unitig batch handed unchanged to a fresh count table, the
    abundance call and the per-record sketches."""
    k, path, pre = case.k, case.path, case.pre
    d = draw_dbg(rng)
    mc = d["min_count"]
    what = f"dbg {d}"
    t, ra, rt, items = sess.counted(case)
    keys, counts, m = dbg_graph(case, d)
    with nt.KmerSet.from_table(t, mc) as s, nt.KmerGraph(s) as g:
        _eq(s.items()[0], keys, what + " keys of the set")
        _, (seq, n_bytes, offsets, n_records) = hold_graph(g, m, len(keys), what)
        if d["release"]:
            g.release()
        if n_records == 0:
            return what
        spelled = [u.encode() for u in m.spelled]
        with nt.KmerTable(k, path, max(n_bytes, 16), sess.ctx) as fresh:
            fresh.count_device(seq, n_bytes, pre)
            got = fresh.items()
            _eq(got[0], keys, what + " recount keys")
            _eq(got[1], np.ones(len(keys), dtype=np.uint64), what + " recount counts")
        rows = _host(ra.run_device(seq, n_bytes, offsets, n_records, pre, min_count=mc))
        _eq(rows, A.rows(spelled, items, k, path, pre, mc), what + " abundance of the unitigs")
        _eq(rows[:, 1], rows[:, 0], what + " every k-mer of a unitig is present")
        _eq(rows[:, 0], m.unitig_rows[:, 1], what + " k-mers per unitig")
        rmh = sess.rmh(case.stage, k, path, dict(scaled=1), 0)
        rmh.run_device(seq, n_bytes, offsets, n_records, pre)
        got = rmh.sketches()
        _eq_csr(got, RM.sketches(spelled, k, path, pre, scaled=1), what + " sketches of the unitigs")
        _eq(np.diff(got[0].astype(np.int64)), m.unitig_rows[:, 1].astype(np.int64), what + " hashes per unitig")
    return what


def _eq_screen(got, want, what):
    for name, g, w in zip(("rows", "hits", "single"), got, want):
        if g is not None:
            _eq(_host(g), w, f"{what} {name}")


def check_colors(sess, case, rng):
    """An index built colour by colour through tables, sets and per-key masks; the batch screened with and without the quality stream and
    d_single, a prefix, the census; then the trimmer's compacted device batch screened as it is."""
    k, path, pre, cutoff = case.k, case.path, case.pre, case.cutoff
    d = draw_colors(rng, case)
    model, steps = colors_steps(case, d)
    what = f"colors n_colors {d['n_colors']} routes {d['routes']} star {d['star']} dead {d['dead']} trim {d['trim']}"
    recs, buf, off, n = case.records, case.buf(), case.offsets(), len(case.records)
    dev, dq, d_off = upload(buf), upload(case.qual_stream().tobytes(), fill=0xFF), _dev_u64(off)
    q = dict(d_qual=dq, quality_cutoff=cutoff)
    values = {False: colors_values(case, False), True: colors_values(case, True)}
    kc = sess.handle((case.stage, "colors", k, path, d["n_colors"]), lambda: nt.KmerColors(k, path, d["n_colors"], TABLE_CAPACITY, sess.ctx))
    kc.reset()
    scratch = sess.scratch_table(case.stage, k, path)
    star_t = star_ra = None
    try:
        lists = [st for st in steps if st[0] != "masks"]
        for route, c, mc, gbuf in lists:
            t = scratch
            if c == d["star"]:
                t = star_t = nt.KmerTable(k, path, max(len(gbuf), 16), sess.ctx)
            t.reset()
            g_dev = upload(gbuf)
            t.count_device(g_dev, len(gbuf), pre)
            sess.ctx.synchronize()
            if route == "table":
                kc.add(t, c, mc)
            else:
                with nt.KmerSet.from_table(t, mc) as ks:
                    kc.add(ks, c)
        if star_t is not None:   # before any mask is added: colour `star` is the table's keys with count >= its min_count
            star_ra = nt.ReadAbundance(star_t)
            hits = _host(kc.run_device(dev, len(buf), d_off, n, pre, single=False)[1])
            present = _host(star_ra.run_device(dev, len(buf), d_off, n, pre, min_count=d["min_counts"][d["star"]]))[:, 1]
            _eq(hits[:, d["star"]], present, what + " hits of the star colour and n_present of its table")
        for _, _, _, (keys, masks) in steps[len(lists):]:
            kc.add_masks(keys, masks)
    finally:
        if star_ra is not None:
            star_ra.close()
        if star_t is not None:
            star_t.close()
    for use_q in (False, True):
        want = KM.screen_values(values[use_q], model)
        for single in (True, False):
            got = kc.run_device(dev, len(buf), d_off, n, pre, single=single, **(q if use_q else {}))
            _eq_screen(got, want, what + f" quality {use_q} single {single}")
    m = d["prefix"]
    got = kc.run_device(dev, int(off[m]), d_off, m, pre, **(q if d["prefix_q"] else {}))
    _eq_screen(got, KM.screen_values(values[d["prefix_q"]][:m], model), what + f" first {m} records")
    kc.release()
    st = kc.stats()
    _eq([st["n_dropped"], st["n_keys"], st["n_masked_bits"]], [0, model.n_keys, model.n_masked_bits], what + " census")
    _eq(st["per_color"], model.per_color(), what + " per_color")
    # the chain: the trimmer's compacted batch, as the device wrote it
    t, ra, rt, items = sess.counted(case)
    mode, mc, ml = d["trim"]
    want_rows, want = trim_chain(case, items, d["trim"])
    d_rows = rt.run_device(dev, len(buf), d_off, n, pre, min_count=mc, mode=mode, min_length=ml, **q)
    _eq(_host(d_rows), want_rows, what + " trim rows")
    out = rt.compact_device(dev, len(buf), d_off, n, d_rows, dq)
    _eq(out[1], want[1], what + " compacted n_bytes")
    n_out = len(want[3])
    if n_out:
        o_recs, o_quals, _ = compacted_records(case, want_rows, want)
        got = kc.run_device(out[0], out[1], out[2], n_out, pre, d_qual=out[4], quality_cutoff=cutoff)
        _eq_screen(got, KM.screen(o_recs, model, k, path, pre, o_quals, cutoff), what + " screen of the compacted batch")
    return what


ML_FIELDS = ("offsets", "pos", "values", "strand", "span")


def _eq_ml(got, want, what):
    for name, g, w in zip(ML_FIELDS, got, want):
        _eq(np.asarray(g).astype(np.uint64), np.asarray(w).astype(np.uint64), f"{what} {name}")


class _DeviceView:
    """`n` words of `typestr` at a device address, for torch.as_tensor."""

    def __init__(self, address, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (address, False), "version": 2}


def _ml_device_result(ml, n_records):
    """The held result cloned where it lies on the device, in the form of read()."""
    import torch
    d_off, d_pos, d_val, d_info, n = ml.device_arrays()
    clone = lambda a, m, t: torch.as_tensor(_DeviceView(a, m, t), device="cuda").clone().cpu().numpy() if m else np.zeros(0, dtype=t)   # noqa: E731
    info = clone(d_info, n, "<i4").view(np.uint32)
    return (clone(d_off, n_records + 1, "<i8").view(np.uint64), clone(d_pos, n, "<i8").view(np.uint64), clone(d_val, n, "<i8").view(np.uint64),
            (info & 1).astype(np.uint8), info >> 1)


def _ml_core_digest(ctx, dev, n_bytes, k, w, path, pre):
    """What the core's windowed-minimizer reduce folds on the same device buffer (w = 256 does not fit the flags of reduce_device)."""
    ctx.accum_reset()
    if w <= 255:
        ctx.reduce_device(dev, n_bytes, k, path, pre, w=w)
    else:
        ctx.minimizers_reduce_device(dev, n_bytes, k, w, path, pre)
    return ctx.accum_read()


def check_minimizer_list(sess, case, rng):
    """One handle per case: all five CSR fields without and with the quality stream, the statistics and the result on the device each
    time; the digest against the core's (a canonical path in LEX order); a prefix of the records; then a second, smaller case, whose
    result replaces the one held."""
    k, path, pre, cutoff = case.k, case.path, case.pre, case.cutoff
    w, order = case.extra["w"], case.extra["order"]
    d = draw_ml(rng, case)
    second = ml_second_case(rng, case, d)
    what = f"minimizer_list w {w} order {order} {d}"
    buf, off, n = case.buf(), case.offsets(), len(case.records)
    dev, dq, d_off = upload(buf, fill=ord("A")), upload(case.qual_stream().tobytes(), fill=0xFF), _dev_u64(off)
    q = dict(d_qual=dq, quality_cutoff=cutoff)

    def held(ml, want, n_records, name):
        _eq_ml(ml.read(), want, name)
        st = ml.stats()
        _eq([st["n_records"], st["n_entries"], st["n_windows"], st["n_chunks"]], [n_records, want[1].size, int(want[4].sum()), 1], name + " stats")
        _eq_ml(_ml_device_result(ml, n_records), want, name + " on the device")

    with nt.MinimizerList(k, path, w, order, sess.ctx) as ml:
        for use_q in (False, True):
            name = what + f" quality {use_q}"
            want = ml_want(case, use_q)
            ml.run_device(dev, len(buf), d_off, n, pre, **(q if use_q else {}))
            held(ml, want, n, name)
            if not use_q and order == MM.LEX and path != BITS:
                got = ml.read()
                core = _ml_core_digest(sess.ctx, dev, len(buf), k, w, path, pre)
                if not MM.same_digest(MM.digest(got[2], got[3], got[4], k), core):
                    raise Mismatch(name + " digest against the core's windowed-minimizer reduce")
        m = d["prefix"]   # the bytes after the prefix are readable and are not input
        ml.run_device(dev, int(off[m]), d_off, m, pre, **(q if d["prefix_q"] else {}))
        held(ml, ml_want(case, d["prefix_q"], m), m, what + f" first {m} records")
        if d["trim"]:
            ml.trim()
        buf2, n2 = second.buf(), len(second.records)
        dev2, dq2 = upload(buf2, fill=ord("A")), upload(second.qual_stream().tobytes(), fill=0xFF)
        kw = dict(d_qual=dq2, quality_cutoff=second.cutoff) if d["second_q"] else {}
        ml.run_device(dev2, len(buf2), _dev_u64(second.offsets()), n2, pre, **kw)
        held(ml, ml_want(second, d["second_q"]), n2, what + " the second, smaller case")
    return what


# ---- the map_reads stage: seeds, chains, mappings and alignments as ReadMapper hands them on --------------------------------------------

MAP_KS = (11, 15, 16, 17, 21)            # the k of `KS` that leave room for seeds
MAP_PRES = tuple(p for path, p in PATH_PRES if path == BITS_CANON)
MAP_COPIES = (3, 4, 6)                   # copies of the dispersed family of a plain case
MAP_FAMILY_COPIES = (12, 16)             # and of a "repeat family" case: one read gets more than MP_LDS_CHAINS chains
MAP_FAMILY_W = (5, 11)
MAP_FAMILY_LEN = 200
THIN_SIZES = (63, 64, 65, 127, 128, 129)   # n and m of the between parts the thinned chains aim at: the 64-row strips of aln_dp_kernel
THIN_PER_CLASS = 3                         # chains thinned per class and case: the DP of the host model is what a thinned chain costs
U32_MAX, I31_MAX = (1 << 32) - 1, (1 << 31) - 1


def _pick(rng, values):
    """One of `values`, whose first is the default: that one four times in ten, else any."""
    return values[0] if rng.random() < 0.4 else values[int(rng.integers(0, len(values)))]


def draw_map_extra(rng, k) -> dict:
    """What a map_reads case fixes before its sequences: the class, (w, order), the copies of the planted family, and one value per
    parameter of SeedIndex.match, AnchorChains.run, ChainMappings.run and ChainAlignments.run - the default, both ends of the range the
    model's check_params accepts, and the values next to the kernels' constants (CH_RING = 512 and the 64-lane strip for h; max_dist and
    bw of tens of bases, which real gaps equal)."""
    cls = "repeat_family" if rng.random() < 0.25 else "plain"
    if cls == "plain":
        names = list(ML_W_CLASSES)
        ws = ML_W_CLASSES[names[int(rng.integers(0, len(names)))]]
        w, copies = int(ws[int(rng.integers(0, len(ws)))]), int(rng.choice(MAP_COPIES))
    else:
        w, copies = int(rng.choice(MAP_FAMILY_W)), int(rng.choice(MAP_FAMILY_COPIES))
    max_dist = _pick(rng, (5000, 1, I31_MAX, 30, 50, 80))
    bw = _pick(rng, (500, 0, 3, 10, 20, None))
    e = dict(cls=cls, w=w, order=int(ML_ORDERS[int(rng.integers(0, len(ML_ORDERS)))]), copies=copies,
             max_occ=_pick(rng, (0, 1, 2, copies - 1, copies)), max_dist=max_dist, bw=max_dist if bw is None else min(bw, max_dist),
             h=_pick(rng, (64, 1, 2, 63, 65, 512)), min_score=_pick(rng, (40, 1, k, k + 1, U32_MAX)), min_cnt=_pick(rng, (3, 1, 2, U32_MAX)),
             mask_level=_pick(rng, (0.5, 0.0, 1.0)), pri_ratio=_pick(rng, (0.8, 0.0, 1.0)), best_n=_pick(rng, (5, 0, 1)),
             a=_pick(rng, (2, 1, 255)), b=_pick(rng, (4, 1, 255)), q=_pick(rng, (4, 0, 255)), e=_pick(rng, (2, 1, 255)),
             band_pad=_pick(rng, (64, 0, 1, 16)), max_seg=_pick(rng, (2048, 1, 4095, 30, 100)))
    if cls == "repeat_family":   # every few anchors a chain of their own, and each is kept
        e["max_dist"] = int(rng.choice((3, 5)))
        e.update(bw=min(e["bw"], e["max_dist"]), min_cnt=1, min_score=int(rng.choice((1, k))), max_occ=int(rng.choice((0, copies))))
        if e["pri_ratio"]:       # the tiny chains of the copies tie in score: at 1 a secondary is eligible at exactly the ratio of mp_eligible
            e["pri_ratio"] = 1.0
    return e


MAP_CALL = ("max_occ", "max_dist", "bw", "h", "min_score", "min_cnt", "mask_level", "pri_ratio", "best_n", "a", "b", "q", "e", "band_pad", "max_seg")


def map_kw(case) -> dict:
    """The keyword arguments of ReadMapper.map_aligned of a case."""
    return {name: case.extra[name] for name in MAP_CALL}


def _revcomp(a):
    return COMP[a[::-1]]


def _edited(rng, a, sub, indel):
    """`a` with substitutions at rate `sub` and insertions and deletions of 1 .. 3 bases at rate `indel`."""
    a = a.copy()
    hit = rng.random(a.size) < sub
    a[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    out, at = [], 0
    for p in np.flatnonzero(rng.random(a.size) < indel).tolist():
        if p < at:
            continue
        out.append(a[at:p])
        n = int(rng.integers(1, 4))
        if rng.random() < 0.5:
            out.append(ACGT[rng.integers(0, 4, n)])
            at = p
        else:
            at = p + n
    out.append(a[at:])
    return np.concatenate(out).astype(np.uint8)


def _ref_cut(rng, refs, L, r=None, where=None):
    """(bases, reference, start) of a cut of at most L bases of one reference record: anywhere, at its head or at its tail."""
    r = int(rng.integers(0, len(refs))) if r is None else r
    n = refs[r].size
    L = min(L, n)
    s = 0 if where == "head" else n - L if where == "tail" else int(rng.integers(0, n - L + 1))
    return refs[r][s:s + L].copy(), r, s


def _without(a, at, n):
    """`a` without the n bases from `at` on: a deletion of exactly n."""
    return np.concatenate([a[:at], a[at + n:]])


def make_map_case(rng, k, pre, extra) -> Case:
    """One case of the map_reads stage: `ref_records` are one to four reference records cut from a random genome with a tandem repeat, a
    dispersed family of diverged copies on both strands, N runs and lower-case stretches planted; `records` are the reads, `kinds` what
    each was made as, `origins` (reference, start, reverse) of the reads cut from a region nothing was planted in, substitutions only."""
    c = Case(k, BITS_CANON, pre, "map_reads", extra)
    w, copies, family = extra["w"], extra["copies"], extra["cls"] == "repeat_family"
    fam_len = MAP_FAMILY_LEN if family else int(rng.integers(120, 301))
    n = int(rng.integers(2500, 4501)) + copies * fam_len
    g = ACGT[rng.integers(0, 4, n)].copy()
    planted = np.zeros(n, dtype=bool)
    unit = ACGT[rng.integers(0, 4, int(rng.integers(5, 31)))]
    t_len = int(rng.integers(100, 251))
    # Now and then a tandem repeat of 64 copies and what a k-mer takes: a reference position of it then matches 63, 64 or 65 read
    # positions, so the nearest anchor on a diagonal lies 64 anchors back in the sorted order - a whole wave of the chain recurrence.
    # (One minimizer per period, w >= 3: at w = 1 or 2 a read of it alone would make tens of thousands of anchors.)
    long_tandem = not family and w >= 3 and rng.random() < 0.25
    if long_tandem:
        unit = ACGT[rng.integers(0, 4, int(rng.integers(3, 7)))]
        t_len = unit.size * (64 + -(-(k - 1) // unit.size) + 1)
    t_at = int(rng.integers(0, n - t_len))
    g[t_at:t_at + t_len] = np.resize(unit, t_len)
    planted[t_at:t_at + t_len] = True
    fam, win, fam_at = ACGT[rng.integers(0, 4, fam_len)], n // copies, []
    for j in range(copies):
        s = j * win + int(rng.integers(0, win - fam_len + 1))
        copy = _edited(rng, fam, 0.01 if family else 0.02, 0.0) if j else fam.copy()
        g[s:s + fam_len] = _revcomp(copy) if rng.random() < 0.5 else copy
        planted[s:s + fam_len] = True
        fam_at.append(s)
    for _ in range(int(rng.integers(1, 4))):
        ln, s = int(rng.integers(1, 41)), int(rng.integers(0, n - 40))
        g[s:s + ln] = ord("N")
        planted[s:s + ln] = True
    for _ in range(int(rng.integers(1, 4))):
        ln, s = int(rng.integers(20, 201)), int(rng.integers(0, n - 200))
        g[s:s + ln] |= 0x20
    cuts = [0] + sorted(set(rng.integers(1, n, int(rng.integers(0, 4))).tolist())) + [n]
    refs = [g[a:b] for a, b in zip(cuts, cuts[1:])]
    c.ref_records = [r.tobytes() for r in refs]
    ref_of = lambda p: int(np.searchsorted(cuts, p, side="right")) - 1   # noqa: E731

    plan = []   # (kind, bases, origin)
    add = lambda kind, a, origin=None: plan.append((kind, np.asarray(a, dtype=np.uint8), origin))   # noqa: E731
    for _ in range(int(rng.integers(8, 13)) // (2 if w <= 2 else 1)):   # (at w = 1 every k-mer is a seed: half as many)
        add("cut", _edited(rng, _ref_cut(rng, refs, int(1500 * rng.random() ** 3))[0], float(rng.choice((0.0, 0.01, 0.03))), 0.003))
    for _ in range(3):   # substitutions only, from a region nothing was planted in: the origin is known
        L = int(rng.integers(150, 401))
        for _try in range(20):
            a, r, s = _ref_cut(rng, refs, L)
            if not planted[cuts[r] + s: cuts[r] + s + a.size].any():
                add("unique", _edited(rng, a, 0.01, 0.0), (r, s))
                break
    add("long", _edited(rng, _ref_cut(rng, refs, int(rng.integers(700, 1501)))[0], 0.005, 0.001))
    for turn in range(2):   # a stretch at a high substitution rate with two indels, between clean flanks: its path leaves the diagonal
        a = _ref_cut(rng, refs, int(rng.integers(400, 701)))[0]
        if a.size > 320:
            ln = int(rng.integers(60, 201))
            s = int(rng.integers(60, a.size - ln - 59))
            mid = _edited(rng, a[s:s + ln], 0.3, 0.0)
            # a deletion and an insertion of d bases each, 30 apart, in either order: n = m, and the path between them runs d off the
            # diagonal - on the band's edge where d is band_pad
            d = extra["band_pad"] if 1 <= extra["band_pad"] <= 16 else int(rng.integers(1, 11))
            x, y = ln // 2 - 15, ln // 2 + 15
            ins = ACGT[rng.integers(0, 4, d)]
            mid = np.concatenate([mid[:x], mid[x + d:y], ins, mid[y:]]) if turn else np.concatenate([mid[:x], ins, mid[x:y], mid[y + d:]])
            a = np.concatenate([a[:s], mid, a[s + ln:]])
        add("divergent", a)
    # one indel longer than max_seg, one of exactly bw and one of bw + 1 (a deletion from the read: dr - dq is the indel)
    max_seg, bw, max_dist = extra["max_seg"], extra["bw"], extra["max_dist"]
    for kind, d in (("long_indel", max_seg + 1 + int(rng.integers(0, 3)) if max_seg <= 200 else int(rng.integers(30, 81))),
                    ("bw_indel", bw if 1 <= bw <= 200 else int(rng.integers(1, 21))), ("bw_indel", bw + 1 if bw <= 200 else int(rng.integers(1, 21)))):
        a = _ref_cut(rng, refs, 400 + d)[0]
        add(kind, _without(a, a.size // 2 - d // 2, d) if a.size > d + 100 else a)
    # destroyed blocks whose flanking anchors lie about max_dist apart: the block and the seed behind it are max_dist - (0 .. w) long
    for _ in range(2):
        a = _ref_cut(rng, refs, 600)[0]
        if 20 <= max_dist <= 300 and a.size == 600:
            for s in (150, 350):
                ln = max(max_dist - k - int(rng.integers(0, w + 1)), 1)
                a[s:s + ln] = COMP[a[s:s + ln]]
        add("spacer", a)
    for _ in range(2):   # two references, or two strands of one
        a, r, _ = _ref_cut(rng, refs, int(rng.integers(100, 401)))
        b = _ref_cut(rng, refs, int(rng.integers(100, 401)), r=(r + 1) % len(refs))[0]
        add("chimera", np.concatenate([a, _revcomp(b) if len(refs) == 1 or rng.random() < 0.5 else b]))
    for _ in range(2):
        add("foreign", ACGT[rng.integers(0, 4, int(rng.integers(50, 301)))])
    for where in ("head", "tail", "head", "tail"):
        add(where, _edited(rng, _ref_cut(rng, refs, int(rng.integers(60, 301)), where=where)[0], 0.01, 0.0))
    for L in (0, 1, k - 1, k, k + w - 2, k + w - 1, k + w):
        add("edge", _ref_cut(rng, refs, L)[0])
    for j in rng.integers(0, copies, 2).tolist():   # a copy of the family with its flanks; the tandem repeat with its flanks
        s = max(fam_at[j] - int(rng.integers(0, 80)), cuts[ref_of(fam_at[j])])
        add("family", _edited(rng, g[s:min(s + fam_len + 100, cuts[ref_of(s) + 1])], 0.01, 0.0))
    s = max(t_at - 60, cuts[ref_of(t_at)])
    add("tandem", g[s:min(t_at + t_len + 60, cuts[ref_of(s) + 1])].copy())
    if long_tandem:   # and one copy less of it, without the flank behind
        add("tandem", g[s:min(t_at + t_len - unit.size, cuts[ref_of(s) + 1])].copy())
    else:             # one unit less and two units more in the middle: chains that fork off the best one, and fork again
        a, mid = plan[-1][1], t_at - s + t_len // 2
        if a.size > mid + unit.size:
            add("tandem", _without(a, mid, unit.size))
            add("tandem", np.concatenate([a[:mid], a[mid - 2 * unit.size:mid], a[mid:]]))
    if family:
        add("family_x2", np.concatenate([fam, fam[:fam_len // 2]]))   # (a unit and a half: the mapping model is quadratic in a read's chains)
    junk = junk_bytes(pre)
    order = rng.permutation(len(plan))
    c.origins = []
    for i in order.tolist():
        kind, a, origin = plan[i]
        rev = bool(rng.random() < 0.5)
        if rev:
            a = _revcomp(a)
        if kind not in ("unique", "edge") and a.size and rng.random() < 0.3:   # junk, lower case, U for T
            a = a.copy()
            m = rng.random(a.size)
            a[m < 0.1] |= 0x20
            sel = m > 0.99
            a[sel] = junk[rng.integers(0, junk.size, int(sel.sum()))]
            a[(m > 0.97) & (m <= 0.99) & (a == ord("T"))] = ord("U")
        c.records.append(a.tobytes())
        c.kinds.append(kind)
        c.classes.append(None)
        c.origins.append(None if origin is None else origin + (rev,))
    for _ in range(2):   # exact duplicates
        j = int(rng.integers(0, len(c.records)))
        c.records.append(c.records[j])
        c.kinds.append("dup")
        c.classes.append(None)
        c.origins.append(c.origins[j])
    return c


class Pipeline:
    """The host truth of one run of ReadMapper.index and .map_aligned, stage by stage (`pipeline_want`)."""


def _list_of(buf, off, case):
    """The minimizer list of a packed batch as the seed index takes it: (offsets, pos, values, span << 1 | strand)."""
    ent = MM.entries_of(buf, case.k, case.extra["w"], BITS_CANON, case.pre, case.extra["order"])
    o, pos, values, strand, span = MM.csr(ent, off, len(buf), case.k)
    return SI.as_list(o, pos, values, (span.astype(np.uint32) << np.uint32(1)) | strand.astype(np.uint32))


def map_params(case):
    """(chain, mapping, alignment) parameters of a case as the three models take them."""
    e = case.extra
    return (CH.Params(case.k, e["max_dist"], e["bw"], e["h"], e["min_score"], e["min_cnt"]),
            MP.Params(case.k, int(round(e["mask_level"] * 1000)), int(round(e["pri_ratio"] * 1000)), e["best_n"], e["min_score"]),
            AL.Params(case.k, e["a"], e["b"], e["q"], e["e"], e["band_pad"], e["max_seg"], 0))


def pipeline_want(case, n_reads=None) -> Pipeline:
    """What the four handles of a ReadMapper hold after index() of the case's references and map_aligned() of its first `n_reads` reads
    (None: all), from bytes alone: both minimizer lists from `_minimizer_list_model`, the anchors from `_seed_index_model.match`, the
    chains from `_chain_model.chain`, the marks from `_mapping_model.run`, the alignments of the reported chains from `_align_model.run`,
    and each stage's stats.  Cached on the case."""
    cache = case.__dict__.setdefault("_want", {})
    if n_reads in cache:
        return cache[n_reads]
    p = Pipeline()
    m = len(case.records) if n_reads is None else n_reads
    ref_buf, ref_off = pack(case.ref_records), T.offsets(case.ref_records)
    off = case.offsets()[:m + 1]
    buf = case.buf()[:int(off[m])]
    p.refs, p.reads = AL.Batch(np.frombuffer(ref_buf, dtype=np.uint8), ref_off), AL.Batch(np.frombuffer(buf, dtype=np.uint8), off)
    p.ref_list, p.read_list = _list_of(ref_buf, ref_off, case), _list_of(buf, off, case)
    p.index = SI.Index(p.ref_list)
    status, p.seeds, p.n_anchors = SI.match(p.index, p.read_list, case.extra["max_occ"])
    assert status == SI.OK
    a_off, ref, rev, rpos, qpos, _ = p.seeds
    p.anchors = CH.as_anchors(a_off, (ref << np.uint32(1)) | rev.astype(np.uint32), rpos, qpos)
    p.cp, p.mp, p.ap = map_params(case)
    p.chains = CH.chain(p.anchors, p.cp)
    ch = p.chains
    p.mch = MP.Chains(ch.c_offsets, ch.chain_rows, ch.m_offsets, ch.members, rpos, qpos)
    p.marks = MP.run(p.mch, p.mp)
    p.inp = AL.Input(p.refs, p.reads, AL.Chains(*p.mch), p.marks.out)
    p.aln, p.aligned = AL.run(p.inp, p.ap)
    p.stats = dict(seeds=SI.stats(p.index, p.read_list, p.n_anchors), chains=CH.stats(p.anchors, p.cp, p.chains),
                   mappings=MP.stats(p.mch, p.marks), alignments=AL.stats(p.inp, p.ap, p.aln, p.aligned))
    cache[n_reads] = p
    return p


def thin_classes(n, m):
    """The classes of THIN_SIZES a between part of n x m meets: ("n", size), ("m", size), and "cross" where n != m lie across 64."""
    out = [("n", n)] * (n in THIN_SIZES) + [("m", m)] * (m in THIN_SIZES)
    return out + ["cross"] * (min(n, m) >= 1 and min(n, m) < 64 < max(n, m))


def thinned_input(case):
    """(input, sizes): the second alignment input of a case.  Its chains are the reported chains of the whole run, entry by entry in the
    order reported, each without the members strictly between one pair (i, j) of its members - first and last are kept, order and
    dr, dq >= 1 survive - so that members i and j, which lay a few bases apart with minimizers between them, bound one between part of
    n x m bases.  The pair is found by search over all member pairs of the chain: one whose part (at most max_seg) meets the class of
    `thin_classes` that the case's earlier chains met least often, and fewer than THIN_PER_CLASS times; a chain without such a pair stays
    whole.  sizes: (n, m) of the part
    made, per chain (None: whole).  The anchors are the run's own; the selection is every chain."""
    p = pipeline_want(case)
    ch, k, max_seg = p.inp.chains, case.k, case.extra["max_seg"]
    seen, rows, members, m_offsets, sizes = {}, [], [], [0], []
    for c in p.marks.out.tolist():
        m = np.asarray(AL.members_of(ch, c), dtype=np.int64)
        if m.size < 3:   # nothing lies between its ends
            rows.append(ch.chain_rows[c].copy())
            members += m.tolist()
            m_offsets.append(len(members))
            sizes.append(None)
            continue
        r, q = ch.rpos[m].astype(np.int64), ch.qpos[m].astype(np.int64)
        if int(ch.chain_rows[c, 2]) & 1:
            q = -q
        dr, dq = r[None, :] - r[:, None], q[None, :] - q[:, None]   # [i, j]: from member i to member j
        m0 = np.minimum(np.minimum(dr, dq), k)
        n_, m_ = dr - m0, dq - m0
        ok = (np.arange(m.size)[None, :] > np.arange(m.size)[:, None] + 1) & (np.maximum(n_, m_) <= max_seg)
        cand = {}
        for i, j in np.argwhere(ok & (np.isin(n_, THIN_SIZES) | np.isin(m_, THIN_SIZES) | ((np.minimum(n_, m_) >= 1) & (np.minimum(n_, m_) < 64) & (np.maximum(n_, m_) > 64)))).tolist():
            for cls in thin_classes(int(n_[i, j]), int(m_[i, j])):
                cand.setdefault(cls, (i, j))
        row = ch.chain_rows[c].copy()
        cand = {x: pair for x, pair in cand.items() if seen.get(x, 0) < THIN_PER_CLASS}
        if cand:
            cls = min(cand, key=lambda x: (seen.get(x, 0), str(x)))
            i, j = cand[cls]
            for x in thin_classes(int(n_[i, j]), int(m_[i, j])):
                seen[x] = seen.get(x, 0) + 1
            m = np.concatenate([m[:i + 1], m[j:]])
            sizes.append((int(n_[i, j]), int(m_[i, j])))
        else:
            sizes.append(None)
        row[1] = m.size
        rows.append(row)
        members += m.tolist()
        m_offsets.append(len(members))
    c_offsets = np.concatenate([[0], np.cumsum(np.diff(p.marks.out_offsets.astype(np.int64)))]).astype(np.uint64)
    chains = AL.Chains(c_offsets, np.asarray(rows, dtype=np.uint32).reshape(-1, 8), np.asarray(m_offsets, dtype=np.uint64),
                       np.asarray(members, dtype=np.uint32), ch.rpos, ch.qpos)
    return AL.Input(p.refs, p.reads, chains, np.arange(len(rows), dtype=np.uint32)), sizes


def thinned_want(case):
    """(input, sizes, result, chains) of the thinned-chain alignment: `_align_model.run` on the arrays of `thinned_input`.  Cached."""
    cache = case.__dict__.setdefault("_want", {})
    if "thin" not in cache:
        inp, sizes = thinned_input(case)
        cache["thin"] = (inp, sizes) + _thinned_run(case, inp, sizes)
    return cache["thin"]


def _thinned_run(case, inp, sizes):
    """`_align_model.run(inp, p)`, entry by entry as it builds its result, but for a chain that stayed whole the model's answer of the
    pipeline run is taken: the same chain over the same anchors and sequences has the same alignment (tests/test_lib_fuzz_inputs.py
    holds this shortcut to the plain `run`)."""
    want, p = pipeline_want(case), map_params(case)[2]
    rows, scores, g_offsets, cigar, chains, cache = [], [], [0], [], [], {}
    for s, size in enumerate(sizes):
        got = want.aligned[s] if size is None else AL.chain(inp, s, p, None, cache)
        chains.append(got)
        count = lambda op: sum(n for o, n in got.runs if o == op)   # noqa: E731
        rows.append([AL.TOO_LONG, 0, 0, 0, 0, 0, 0, 0] if got.too_long else
                    [AL.ALIGNED, len(got.runs), count(AL.OP_EQ), count(AL.OP_X), count(AL.OP_I), count(AL.OP_D),
                     sum(1 for o, _ in got.runs if o in (AL.OP_I, AL.OP_D)), 0])
        scores.append(0 if got.too_long else AL.score_of(got.runs, p))
        cigar += [n << 4 | op for op, n in got.runs]
        g_offsets.append(len(cigar))
    return AL.Result(np.asarray(rows, dtype=np.uint32).reshape(-1, 8), np.asarray(scores, dtype=np.int64), np.asarray(g_offsets, dtype=np.uint64),
                     np.asarray(cigar, dtype=np.uint32)), chains


def draw_map(rng, case) -> dict:
    """The checker's draw of a map_reads case: the prefix of the reads that is mapped again on the same handles."""
    return dict(prefix=int(rng.integers(1, len(case.records) // 6 + 1)))   # (the models are what a case costs: a sixth at the most)


def _dev_u32(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    return t


def _eq_stats(got, want, names, what):
    _eq([got[n] for n in names if n != "device_bytes"], [want[n] for n in names if n != "device_bytes"], what + " stats")


def _hold_pipeline(rm, p, what):
    """Every field the four handles read back and every stats word but device_bytes, against `p`: the first unequal stage, field and
    index goes into the Mismatch."""
    for stage, handle, names, want, stats_names in (("seeds", rm.seeds, SI.FIELDS, p.seeds, SI.STATS), ("chains", rm.chains, CH.FIELDS, p.chains, CH.STATS),
                                                    ("mappings", rm.mappings, MP.FIELDS, p.marks, MP.STATS),
                                                    ("alignments", rm.alignments, AL.FIELDS, p.aln, AL.STATS)):
        got = handle.read()
        _eq(len(got), len(names), f"{what} {stage} fields")
        for name, g, w_ in zip(names, got, want):
            _eq(g, w_, f"{what} {stage} {name}")
        _eq_stats(handle.stats(), p.stats[stage], stats_names, f"{what} {stage}")


def _hold_returned(got, p, what):
    """What ReadMapper.map_aligned returns - the structured mappings and the four arrays of the alignments - against `p`."""
    mappings, rest = got[0], got[1:]
    out, rows = p.marks.out.astype(np.int64), p.marks.rows
    _eq(mappings.size, out.size, what + " reported rows")
    sel = rows[out]
    _eq(mappings["read"], np.repeat(np.arange(p.marks.out_offsets.size - 1), np.diff(p.marks.out_offsets.astype(np.int64))), what + " read")
    for name in ("qs", "qe", "rs", "re", "score", "cnt", "mlen", "blen", "mapq"):
        _eq(mappings[name], sel[:, MP.W[name]], f"{what} {name}")
    _eq(mappings["ref"], sel[:, MP.W["ref_rev"]] >> 1, what + " ref")
    _eq(mappings["strand"] == b"-", (sel[:, MP.W["ref_rev"]] & 1) == 1, what + " strand")
    _eq(mappings["primary"], (sel[:, MP.W["flags"]] & MP.PRIMARY) != 0, what + " primary")
    for name, g, w_ in zip(AL.FIELDS, rest, p.aln):
        _eq(g, w_, f"{what} alignments {name}")


def check_map_reads(sess, case, rng):
    """index() and map_aligned() on the ReadMapper the session keeps for (k, w, order) - its six handles hold what the case before left -
    held field by field to `pipeline_want`; a prefix of the reads on the same handles; then the thinned chains through a ChainAlignments
    of the session as plain device arrays.  Every upload stays alive until the context is synchronised."""
    k, pre, e = case.k, case.pre, case.extra
    d = draw_map(rng, case)
    what = f"map_reads {e} {d}"
    rm = sess.handle(("map_reads", "mapper", k, e["w"], e["order"]), lambda: nt.ReadMapper(k, e["w"], e["order"], sess.ctx))
    al = sess.handle(("map_reads", "aligner"), lambda: nt.ChainAlignments(sess.ctx))
    ref_buf, buf, off = pack(case.ref_records), case.buf(), case.offsets()
    r_dev, r_off = upload(ref_buf, fill=ord("A")), _dev_u64(T.offsets(case.ref_records))
    q_dev, q_off = upload(buf, fill=ord("A")), _dev_u64(off)
    keep = [r_dev, r_off, q_dev, q_off]
    rm.index(r_dev, len(ref_buf), r_off, len(case.ref_records), pre)
    n = len(case.records)
    got = rm.map_aligned(q_dev, len(buf), q_off, n, pre, **map_kw(case))
    want = pipeline_want(case)
    _hold_pipeline(rm, want, what + " whole")
    _hold_returned(got, want, what + " whole, as map_aligned returns it")
    m = d["prefix"]   # the bytes after the prefix are readable and are not input
    got = rm.map_aligned(q_dev, int(off[m]), q_off, m, pre, **map_kw(case))
    _hold_pipeline(rm, pipeline_want(case, m), what + f" first {m} reads")
    _hold_returned(got, pipeline_want(case, m), what + f" first {m} reads, as map_aligned returns them")
    inp, _, t_want, t_chains = thinned_want(case)
    ch = inp.chains
    t_dev = [_dev_u64(ch.c_offsets), _dev_u32(ch.chain_rows), _dev_u64(ch.m_offsets), _dev_u32(ch.members), _dev_u32(ch.rpos), _dev_u32(ch.qpos),
             _dev_u32(inp.sel)]
    keep += t_dev
    al.run((r_dev, len(ref_buf), r_off, len(case.ref_records)), (q_dev, len(buf), q_off, n), tuple(t_dev[:4]), tuple(t_dev[4:6]), t_dev[6],
           **map_params(case)[2]._asdict())
    for name, g, w_ in zip(AL.FIELDS, al.read(), t_want):
        _eq(g, w_, f"{what} thinned chains {name}")
    _eq_stats(al.stats(), AL.stats(inp, map_params(case)[2], t_want, t_chains), AL.STATS, what + " thinned chains")
    sess.ctx.synchronize()
    del keep
    return what


CHECKERS = {"count": check_count, "count_wide": check_count, "minhash": check_minhash, "minhash_wide": check_minhash,
            "abundance": check_abundance, "trim": check_trim, "record_minhash": check_record_minhash, "kmer_sets": check_kmer_sets,
            "kmer_sets_wide": check_kmer_sets, "dbg": check_dbg, "colors": check_colors,
            "minimizer_list": check_minimizer_list, "map_reads": check_map_reads}


def run_case(sess, seed, stage, it):
    """Case `it` of a stage on the device.  A failure carries what the tool needs to replay it."""
    rng, case = draw_case(seed, stage, it)
    try:
        CHECKERS[stage](sess, case, rng)
    except Exception as e:
        kinds = sorted(set(case.kinds))
        raise Mismatch(f"MISMATCH seed {seed} it {it} stage {stage} ({case.tag()} kinds {kinds}): {type(e).__name__}: {e}") from e
    return case


def run_slice(sess, stage):
    seed, n = SLICES[stage]
    for it in range(1, n + 1):
        run_case(sess, seed, stage, it)


def dump(case, path):
    """The case as an .npz: packed query batch, offsets, quality stream, packed reference batch and its offsets, and its parameters."""
    np.savez(path, seq=np.frombuffer(case.buf(), dtype=np.uint8), offsets=case.offsets(), qual=case.qual_stream(),
             ref=np.frombuffer(pack(case.ref_records), dtype=np.uint8), ref_offsets=T.offsets(case.ref_records),
             params=np.array([case.k, case.path, case.pre, case.cutoff]), kinds=np.array(case.kinds), stage=np.array(case.stage),
             extra=np.array(repr(case.extra)))
