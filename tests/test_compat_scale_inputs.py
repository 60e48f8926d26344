"""The inputs of tests/test_gpu_compat_scale.py are past the thresholds they aim at - proven without a GPU, from the input builders
(tests/_compat_scale.py), the oracle, the constants in the source text and those csrc/ntk_compat_plan.hpp states when compiled.  A changed constant fails here rather than silently
un-covering a branch of compact_scan_kernel, cp_scan_kernel, the planes kernels' tile loop, grid_for's cap or the long-record hand-over."""
import os
import re

import numpy as np
import pytest

import oracle as O
import _compat_plan as P
import _compat_scale as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "needletail_amd", "csrc")


@pytest.fixture(scope="module")
def src():
    return {name: open(os.path.join(CSRC, name)).read() for name in ("ntk_kernels.hpp", "ntk_api.hip")}


def _const(text, name):
    return int(re.search(rf"\b{name} = (\d+)\b", text).group(1))


@pytest.fixture(scope="module")
def consts(src, tmp_path_factory):
    k, api = src["ntk_kernels.hpp"], src["ntk_api.hip"]
    plan = P.build(tmp_path_factory.mktemp("compat_plan"))   # the default chunk, the long-record threshold and the bank count: asked of the header
    grid = re.search(r"inline unsigned grid_for\(uint64_t items, unsigned block\) \{.*?b > \(1u << (\d+)\) \? \(1u << (\d+)\)", api)
    assert grid.group(1) == grid.group(2)
    return {
        "compact_block": _const(k, "kCompactThreads") * _const(k, "kCompactPerThread"),
        "cp_block": _const(k, "kCpThreads") * _const(k, "kCpWords") * 16,
        "pl_tile": _const(k, "kPlThreads") * _const(k, "kPlPer"),
        "chunk": plan.plan_default_chunk(),
        "long_record": plan.plan_long_record(),
        "banks": plan.plan_banks(),
        "grid_cap_blocks": 1 << int(grid.group(1)),
    }


def test_kernel_constants_are_the_tests(src, consts):
    """The numbers tests/_compat_scale.py aims at, held to the source: block and tile sizes, the one-block scans' 1024 threads, the grid of
    the planes kernels, the default chunk, the long-record threshold, the grid cap and the 256-thread blocks of the element-wise kernels."""
    k, api = src["ntk_kernels.hpp"], src["ntk_api.hip"]
    assert consts["compact_block"] == S.COMPACT_BLOCK_BYTES
    assert re.search(r"kCompactBlockBytes = kCompactThreads \* kCompactPerThread;", k)
    assert consts["cp_block"] == S.CP_BLOCK_POSITIONS
    assert re.search(r"kCpBlockWords = kCpThreads \* kCpWords;", k)
    assert consts["pl_tile"] == S.PL_TILE
    assert re.search(r"kPlTile = kPlThreads \* kPlPer;", k)
    assert consts["chunk"] == S.DEFAULT_CHUNK_BYTES
    assert consts["long_record"] == S.LONG_RECORD
    assert consts["banks"] == S.BANKS
    # ... and the library uses the header's numbers: the ctx's default and its option, the banks it keeps, the hand-over below
    assert re.search(r"uint64_t compat_chunk = kCompatChunkBytes;", api)
    assert re.search(r"c->compat_chunk = value == 0 \? kCompatChunkBytes : \(value < kCompatChunkMin \? kCompatChunkMin : value\);", api)
    assert re.search(r"CompatBank bank\[kCompatBanks\];", api) and not re.search(r"\bkLongRecord = ", api)
    assert consts["grid_cap_blocks"] * 256 == S.GRID_CAP_ITEMS
    # both scans are launched as ONE block of 1024 threads and split their work on that number
    assert re.search(r"hipLaunchKernelGGL\(compact_scan_kernel, dim3\(1\), dim3\(1024\)", api)
    assert re.search(r"hipLaunchKernelGGL\(cp_scan_kernel, dim3\(1\), dim3\(1024\)", api)
    assert re.search(r"const uint32_t per = \(nblocks \+ 1023\) / 1024;", k)
    assert re.search(r"for \(uint64_t b0 = 0; b0 < nblocks; b0 \+= 1024\)", k)
    assert S.SCAN_THREADS == 1024
    # the planes kernels run on n_cu * 8 blocks at most, tile by tile
    assert len(re.findall(r"const dim3 grid\(\(unsigned\)\(tiles < \(uint64_t\)c->n_cu \* 8 \? tiles : \(uint64_t\)c->n_cu \* 8\)\);", api)) == 1
    assert S.PL_BLOCKS_PER_CU == 8
    assert len(re.findall(r"for \(uint64_t tile = blockIdx\.x; tile < n_tiles; tile \+= gridDim\.x\)", k)) >= 3
    # the element-wise kernels of the compat face: 256-thread blocks, capped grid, a grid-stride loop
    assert re.search(r"hipLaunchKernelGGL\(map_reverse_kernel, dim3\(grid_for\(n, 256\)\), dim3\(256\)", api)
    assert re.search(r"hipLaunchKernelGGL\(quality_mask_kernel, dim3\(grid_for\(n, 256\)\), dim3\(256\)", api)
    # the hand-over of ntk_minimizer_batch: the wave kernel skips n > long_record, the host launches the one-block kernel for n > kLongRecord
    assert re.search(r"if \(n > long_record\) continue;", k) and re.search(r"if \(n <= kLongRecord\) continue;", api)


def test_compact_inputs_cross_the_block_scan_split(consts):
    """(a): 1024 blocks (one per thread, the last size without a walk), 1025 (per = 2, most threads idle), and per = 3 twice (a last block
    of one byte / a full last thread); the newline blocks are whole blocks on both sides of the split and keep nothing."""
    blk = consts["compact_block"]
    nblocks = [(n + blk - 1) // blk for n in S.COMPACT_SIZES]
    per = [(b + 1023) // 1024 for b in nblocks]
    assert nblocks[:2] == [1024, 1025] and per == [1, 2, 3, 3]
    assert S.COMPACT_SIZES[2] % blk == 1 and S.COMPACT_SIZES[3] % blk == blk - 5
    for n in S.COMPACT_SIZES:
        a = np.frombuffer(S.compact_input_a(n), dtype=np.uint8)
        assert len(a) == n and len(np.unique(a)) == 256
        ws = np.isin(a, np.frombuffer(b" \t\r\n", dtype=np.uint8)).mean()
        assert 0.04 < ws < 0.09
        blocks = S.compact_newline_blocks(n)
        assert blocks[0] == 0 and blocks[-1] == (n + blk - 1) // blk - 1 and 1023 in blocks and (1024 in blocks) == (n > 1024 * blk)
        for b in blocks:
            piece = bytes(a[b * blk:(b + 1) * blk])
            assert piece and set(piece) == {0x0A}
            assert O.normalize(piece, False)[0] == b"" and O.strip_returns(piece)[0] == b""
        # the neighbours of the split's newline blocks do keep bytes, so an offset that loses a block's count shows
        assert len(O.strip_returns(bytes(a[1022 * blk:1023 * blk]))[0]) > blk // 2
    clean = S.compact_input_b()
    assert len(clean) == S.COMPACT_CLEAN_SIZE == 1024 * blk + 1
    for iupac in (False, True):
        assert O.normalize(clean, iupac) == (clean, False)
    assert O.strip_returns(clean) == (clean, True)


def test_grid_inputs_take_the_second_trip(consts):
    """(b): more items than grid_for's capped grid has threads, fewer than two grids' worth: some threads take a second item, most do not."""
    cap = consts["grid_cap_blocks"] * 256
    assert cap < S.GRID_N < 2 * cap and S.GRID_N % 256 != 0
    seq, qual = S.grid_inputs(100_003)
    assert len(seq) == len(qual) == 100_003 and seq != qual and len(set(seq)) == 256
    masked = O.quality_mask(seq, qual, S.QUALITY_SCORE)
    assert 0.3 < masked.count(b"N") / len(masked) < 0.5   # both outcomes of the compare are common


@pytest.fixture(scope="module")
def cp_record():
    return S.cp_record()


def test_cp_record_crosses_the_scan_carry(consts, cp_record):
    """(c): more than 1024 cp blocks; no item in blocks 1023 and 1024 whether the plane is indexed by window end (bit path) or by window
    start (byte path); items on both sides of them; more than 1000 items beyond the split, so the capacity of the test runs out there."""
    blk = consts["cp_block"]
    assert len(cp_record) == S.CP_RECORD_LEN and S.CP_SPLIT == 1024 * blk
    packed = len(cp_record) + 1                                       # one break byte behind the record
    nblocks = ((packed + 15) // 16 + blk // 16 - 1) // (blk // 16)
    assert nblocks > 1024 + 2
    assert len(cp_record) > consts["chunk"]                           # a chunk of its own at the default chunk size
    n = np.frombuffer(cp_record, dtype=np.uint8) == ord("N")
    assert n[:S.CP_N_STRETCH].all() and n[-S.CP_N_STRETCH:].all() and n[S.CP_SPLIT - S.CP_N_STRETCH // 2: S.CP_SPLIT + S.CP_N_STRETCH // 2].all()
    assert 0 < n[S.CP_N_STRETCH: S.CP_SPLIT - S.CP_N_STRETCH // 2].mean() < 0.001          # sparse N elsewhere
    for (k, canonical) in ((21, True), (32, False)):
        pos = O.bit_kmers_arrays(cp_record, k, canonical)[0]
        block = (pos + np.uint64(k - 1)) // np.uint64(blk)
        assert not np.isin(block, (1023, 1024)).any() and (block == 1022).any() and (block >= 1025).any()
        assert int((pos >= S.CP_SPLIT).sum()) > 1000
    pos = O.canonical_kmers_arrays(cp_record, O.reverse_complement(cp_record), 33)[0]
    block = pos // np.uint64(blk)
    assert not np.isin(block, (1023, 1024)).any() and (block == 1022).any() and (block >= 1025).any()
    batch = S.cp_batch(cp_record)
    assert [len(r) > 0 for r in batch] == [True, True, True, False, True] and batch[1] is cp_record
    assert sum(len(r) + 1 for r in batch[:2]) > consts["chunk"] and sum(len(r) + 1 for r in batch[2:]) < consts["chunk"]


def test_cp_ragged_batch_is_one_chunk_past_the_carry(consts):
    recs = S.cp_ragged_records()
    lens = np.array([len(r) for r in recs])
    packed = int(lens.sum()) + len(recs)
    assert int(lens.sum()) >= S.CP_RAGGED_MIN_BYTES == 20 * S.MI and 10_000 <= len(recs) <= 11_500
    assert consts["chunk"] < packed <= S.CP_RAGGED_CHUNK_BYTES        # several chunks by default, one at the raised option
    assert ((packed + 15) // 16 * 16) // consts["cp_block"] > 1024
    assert lens.min() == 0 and lens.max() == 4000
    flat = b"".join(recs)
    for ch in b"ACGTacgtNn-":
        assert ch in flat
    # records lie over the split: the items on its two sides belong to scan tiles 0 and 1
    offs = np.cumsum(lens + 1)
    assert (offs > 1024 * consts["cp_block"]).sum() > 1000


@pytest.mark.parametrize("cu", [256, 304])
def test_planes_batch_gives_every_block_a_second_tile(consts, cu):
    """(d): at least two tiles for every block of an n_cu * 8 grid and a few blocks with a third; records that begin on a tile boundary,
    one byte before and one after it, among them the first tile that is a block's second; one chunk."""
    tile = consts["pl_tile"]
    recs = S.planes_records(cu)
    lens = np.array([len(r) for r in recs])
    total = int(lens.sum())
    assert total >= S.planes_min_bytes(cu) == (2 * cu * 8 + 3) * 2048 + 777
    tiles, grid = (total + tile - 1) // tile, cu * 8
    assert tiles >= 2 * grid + 3 and tiles < 3 * grid and total % tile != 0
    assert total <= consts["chunk"]
    starts = set(np.concatenate(([0], np.cumsum(lens)[:-1])).tolist())
    forced = S.planes_forced_starts(cu)
    assert tile * grid in forced and tile * grid - 1 in forced and tile * grid + 1 in forced
    assert all(f in starts for f in forced)
    assert lens.min() == 0 and lens.max() <= 4000
    flat = b"".join(recs)
    for ch in b"ACGTacgtNnUu":
        assert ch in flat


def _occurs_twice(seq, rc, w):
    """More than one candidate (window of seq or of its reverse complement) equals w?"""
    i = seq.find(w)
    j = rc.find(w)
    first = i if i >= 0 else j
    assert first >= 0
    return (i >= 0 and j >= 0) or (i >= 0 and seq.find(w, i + 1) >= 0) or (j >= 0 and rc.find(w, j + 1) >= 0)


def test_minimizer_inputs_are_long_and_full_of_ties(consts):
    """(e): hundreds of candidates for each of the 1024 threads, and - from the oracle alone - more than one candidate equal to the winner
    on every tie-heavy input; the batch holds the three lengths around the long-record threshold and more than one long record."""
    inputs = S.minimizer_inputs()
    assert S.MINIMIZER_N == 262_144 + 37
    for name, seq in inputs.items():
        assert S.MINIMIZER_N - 1 <= len(seq) <= S.MINIMIZER_N, name
        assert 2 * (len(seq) - max(S.MINIMIZER_LENGTHS) + 1) // 1024 >= 500
    assert set(inputs["random"]) == set(b"ACGTacgtN")
    ir = inputs["inverted_repeat"]
    assert O.reverse_complement(ir) == ir
    for name in S.MINIMIZER_TIE_HEAVY:
        seq = inputs[name]
        rc = O.reverse_complement(seq)
        for m in S.MINIMIZER_LENGTHS:
            assert _occurs_twice(seq, rc, O.minimizer(seq, m)), (name, m)
    assert _occurs_twice(inputs["random"], O.reverse_complement(inputs["random"]), O.minimizer(inputs["random"], 1))
    recs = S.minimizer_batch_records()
    lens = [len(r) for r in recs]
    lr = consts["long_record"]
    assert lens[1:4] == [lr - 1, lr, lr + 1] and lens[4] == 200_000 and lens[5] == 70_000
    assert sum(n > lr for n in lens) >= 2 and lens[0] < 1024 and lens[-1] < 1024 and min(lens) >= S.MINIMIZER_BATCH_LENGTH
    assert sum(lens) <= consts["chunk"]                               # one chunk: the long records share one d_best
    assert _occurs_twice(recs[4], O.reverse_complement(recs[4]), O.minimizer(recs[4], S.MINIMIZER_BATCH_LENGTH))


def test_first_difference_names_the_place():
    assert S.first_difference(b"abc", b"abc") is None and S.first_difference(b"abc", b"abd") == 2 and S.first_difference(b"ab", b"abc") == 2
    with pytest.raises(AssertionError, match=r"first difference at index 5000 \(block 1\)"):
        S.assert_same(np.arange(6000), np.where(np.arange(6000) == 5000, 0, np.arange(6000)), "x", unit=4096)
    S.assert_same(b"same", b"same", "x")


def test_expected_planes_bit_order():
    v, r, vals = S.expected_planes(np.array([0, 20]), 3, [(np.array([0, 17], dtype=np.uint64), np.array([7, 9], dtype=np.uint64), np.array([0, 1], dtype=np.uint8)),
                                                          (np.array([3], dtype=np.uint64), np.array([5], dtype=np.uint64), np.array([1], dtype=np.uint8))], True)
    assert v.tolist() == [0x8000, 0x4100, 0] and r.tolist() == [0, 0x4100, 0]
    assert vals[0] == 7 and vals[17] == 9 and vals[23] == 5 and int(vals.sum()) == 21
