"""The memory the core owns (csrc/ntk_api.hip on ntk_device_mem.hpp): the scratch of the per-sequence calls, the banks and pinned stages of
the batched calls, the partial rows of a reduce launch and the arrays of a pooled batch - on the paths where a stale pointer or a stale
capacity would show: growing, shrinking, Context.trim() and growing again.  Every result is the oracle's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
import oracle as O  # noqa: E402  (the checker)
from needletail_amd import _lib as NL  # noqa: E402

CSRC = os.path.join(os.path.dirname(os.path.abspath(nt.__file__)), "csrc")
K = M = 21


@pytest.fixture
def ctx():
    assert torch.cuda.is_available(), "these tests need a GPU"
    c = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def assert_stats_equal(a, b, what=""):
    for key in ("n_total", "n_fwd", "n_rc", "sum", "xor"):
        assert a[key] == b[key], (what, key, a[key], b[key])
    assert np.array_equal(a["hist"], b["hist"]), what


def _bytes(rng, n, alphabet):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), n)].tobytes()


# ---- the scratch of the per-sequence calls ---------------------------------------------------------------------------------------

def _sequence_case(n):
    """Input and the oracle's answers for one length: mixed-case bytes with N and line ends, qualities, n packed 21-mers."""
    rng = np.random.default_rng(7000 + n)
    seq = _bytes(rng, n, b"ACGTACGTACGTacgtNn\r\n")
    qual = rng.integers(33, 75, n, dtype=np.uint8).tobytes()
    vals = rng.integers(0, 1 << 2 * K, n, dtype=np.uint64)
    canon = [O.bit_canonical(int(v), K) for v in vals]
    return {"seq": seq, "qual": qual, "vals": vals,
            "normalize": O.normalize(seq, False), "strip": O.strip_returns(seq), "rc": O.reverse_complement(seq),
            "canon": (np.array([c[0] for c in canon], dtype=np.uint64), np.array([c[1] for c in canon], dtype=bool)),
            "mask": O.quality_mask(seq, qual, 53), "minimizer": O.minimizer(seq, M) if n >= M else None}


def _run_sequence_calls(ctx, case):
    seq, n = case["seq"], len(case["seq"])
    assert nt.normalize_opt(seq, False, ctx) == case["normalize"], n
    stripped, borrowed = case["strip"]
    assert nt.strip_returns(seq, ctx) == (seq if borrowed else stripped), n
    assert nt.reverse_complement(seq, ctx) == case["rc"], n
    can, flg = nt.bit_canonical(case["vals"], K, ctx)
    assert np.array_equal(can, case["canon"][0]) and np.array_equal(flg, case["canon"][1]), n
    assert nt.quality_mask(seq, case["qual"], 53, ctx) == case["mask"], n
    if case["minimizer"] is None:   # shorter than m: the reference panics (src/sequence.rs:141), the library answers NTK_ERR_BAD_ARG
        assert NL.lib().ntk_minimizer(ctx._h, seq, n, M, C.create_string_buffer(M)) == 2
    else:
        assert nt.minimizer(seq, M, ctx) == case["minimizer"], n


def test_scratch_grows_shrinks_trims_and_regrows(ctx):
    """One context through lengths 1, 300 (above the 256-byte floor of a scratch buffer), 70 000 (18 compaction blocks of 4096 bytes) and
    300 again, every per-sequence call at each; then trim(), and 70 000 and 1 again on what trim() left.  trim() twice in a row, and on a
    context that has run nothing, is OK."""
    cases = {n: _sequence_case(n) for n in (1, 300, 70_000)}   # the oracle's answers, once per length
    for n in (1, 300, 70_000, 300):
        _run_sequence_calls(ctx, cases[n])
    ctx.trim()
    for n in (70_000, 1):
        _run_sequence_calls(ctx, cases[n])
    ctx.trim()
    ctx.trim()
    _run_sequence_calls(ctx, cases[300])
    with nt.Context(0) as fresh:
        fresh.trim()
        _run_sequence_calls(fresh, cases[300])


# ---- the banks and pinned stages of the batched calls ----------------------------------------------------------------------------

def _ragged_records(seed, n_records):
    rng = np.random.default_rng(seed)
    recs = [_bytes(rng, int(n), b"ACGTACGTACGTACGTacgtNn") for n in rng.integers(0, 401, n_records)]
    recs[1], recs[-1] = b"", _bytes(rng, 400, b"ACGT")   # both ends of the range are there
    return recs


def _batch_case(seed, n_records):
    recs = _ragged_records(seed, n_records)
    long_enough = [r for r in recs if len(r) >= M]
    return {"recs": recs, "long": long_enough,
            "canonical": [O.canonical_kmers_arrays(r, O.reverse_complement(r), K) for r in recs],
            "bit": [O.bit_kmers_arrays(r, K, True) for r in recs],
            "minimizer": [O.minimizer(r, M) for r in long_enough]}


def _run_batched_calls(ctx, case, what):
    recs, can, bit = case["recs"], case["canonical"], case["bit"]
    counts, pos, flg = nt.canonical_kmers_batch(recs, K, ctx)
    assert counts.tolist() == [len(w[0]) for w in can], what
    assert np.array_equal(pos, np.concatenate([w[0] for w in can])) and np.array_equal(flg, np.concatenate([w[1] for w in can])), what
    counts, pos, val, flg = nt.bit_kmers_batch(recs, K, True, ctx)
    assert counts.tolist() == [len(w[0]) for w in bit], what
    for j, got in enumerate((pos, val, flg)):
        assert np.array_equal(got, np.concatenate([w[j] for w in bit])), (what, j)
    pl = nt.canonical_kmers_planes(recs, K, ctx)
    assert pl.total == sum(len(w[0]) for w in can), what
    for i, w in enumerate(can):
        gp, gf = pl.arrays(i)
        assert np.array_equal(gp, w[0]) and np.array_equal(gf, w[1]), (what, i)
    pl = nt.bit_kmers_planes(recs, K, True, ctx)
    assert pl.total == sum(len(w[0]) for w in bit), what
    for i, w in enumerate(bit):
        gp, gv, gf = pl.arrays(i)
        assert np.array_equal(gp, w[0]) and np.array_equal(gv, w[1]) and np.array_equal(gf, w[2]), (what, i)
    assert nt.minimizer_batch(case["long"], M, ctx) == case["minimizer"], what


def test_banks_grow_across_chunk_sizes_and_trim(ctx):
    """60 ragged records of 0..400 bytes in chunks of 64 bytes (a record or a few per chunk: every bank is used and re-used, and grows as
    longer records come), 3 000 such records in one chunk of the default size (a bank and its pinned stage grow well beyond that), trim(),
    and the 60 records in chunks of 64 bytes again on the banks trim() emptied."""
    small, large = _batch_case(11, 60), _batch_case(12, 3000)
    try:
        ctx.set_option(NL.OPT_COMPAT_CHUNK_BYTES, 64)
        _run_batched_calls(ctx, small, "64-byte chunks")
        ctx.set_option(NL.OPT_COMPAT_CHUNK_BYTES, 0)
        _run_batched_calls(ctx, large, "default chunks")
        ctx.trim()
        ctx.set_option(NL.OPT_COMPAT_CHUNK_BYTES, 64)
        _run_batched_calls(ctx, small, "64-byte chunks after trim")
    finally:
        ctx.set_option(NL.OPT_COMPAT_CHUNK_BYTES, 0)


# ---- the partial rows of a reduce launch --------------------------------------------------------------------------------------------

def _to_dev(buf: bytes, fill):
    t = torch.full(((len(buf) + 1023) // 1024 * 1024 + 1024,), fill, dtype=torch.uint8, device="cuda")
    t[: len(buf)] = torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()
    return t


def test_partial_rows_grow_with_the_grid():
    """A k = 21 reduce scan over 65 tiles under set_launch(1, 0), (4, 0) and (0, 0): a launch writes one partial row per block - 1, then
    4, then ceil(65 tiles / 12 waves of a 768-thread block) = 6 - so on a fresh context the rows are re-allocated before the second and
    the third launch.  The same with a quality stream and cutoff.  Each result is the oracle's over the records."""
    tile_bytes = int(re.search(r"constexpr int kTileBytes = (\d+);", open(os.path.join(CSRC, "ntk_tile.hpp")).read()).group(1))
    stride = (tile_bytes - (K - 1)) & ~3            # Sv2Geom<21, true>::kStride: the bytes a tile of the k = 21 reduce scan advances by
    rng = np.random.default_rng(31)
    recs = [_bytes(rng, 150, b"ACGTACGTACGTACGTN") for _ in range(426)]
    quals = [rng.integers(33, 75, 150, dtype=np.uint8).tobytes() for _ in recs]
    buf = b"".join(r + b"\n" for r in recs)
    tiles = (len(buf) + stride - 1) // stride       # tile_count of ntk_plan.hpp
    assert (tile_bytes, stride, len(buf), tiles) == (1024, 1004, 426 * 151, 65) and tiles >= 64
    d_seq = _to_dev(buf, 0x41)
    for cutoff in (0, 40):
        d_qual = _to_dev(b"".join(q + b"\xff" for q in quals), 0) if cutoff else None   # (a record's line end is never masked)
        want = O.reduce_records([O.quality_mask(r, q, cutoff) for r, q in zip(recs, quals)] if cutoff else recs, K,
                                O.PATH_BYTES_CANONICAL, O.PRE_NORMALIZE)
        with nt.Context(0, stream=torch.cuda.current_stream().cuda_stream) as fresh:
            for blocks in (1, 4, 0):
                fresh.set_launch(blocks, 0)
                fresh.reduce_device(d_seq, len(buf), K, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, d_qual=d_qual, quality_cutoff=cutoff, reset=True)
                assert_stats_equal(fresh.accum_read(), want, f"blocks {blocks}, cutoff {cutoff}")


# ---- pooled batches ---------------------------------------------------------------------------------------------------------------------

def test_pooled_batches_keep_their_arrays_and_forget_their_fill(ctx):
    """A released batch goes to the context's pool and the next acquire of up to twice its size gets it back with its arrays: what it was
    filled with - the quality stream above all - is gone.  A request no pooled batch serves gets a fresh one."""
    rng = np.random.default_rng(51)
    recs = [_bytes(rng, int(n), b"ACGTACGTACGTACGTN") for n in (150, 90, 200)]
    quals = [rng.integers(0, 200, len(r), dtype=np.uint8).tobytes() for r in recs]   # (raw bytes: about one in ten is below 20)
    path, pre, cutoff = nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, 20
    masked = O.reduce_records([O.quality_mask(r, q, cutoff) for r, q in zip(recs, quals)], K, O.PATH_BYTES_CANONICAL, O.PRE_NORMALIZE)
    plain = O.reduce_records(recs, K, O.PATH_BYTES_CANONICAL, O.PRE_NORMALIZE)
    assert masked["n_total"] < plain["n_total"]   # the cutoff masks something: a left-over quality stream would show

    def run(batch, with_qual):
        for r, q in zip(recs, quals):
            assert batch.append(r, pre, qual=q if with_qual else None, quality_cutoff=cutoff if with_qual else 0)
        batch.submit(K, path, pre, quality_cutoff=cutoff if with_qual else 0, reset=True)
        batch.wait()
        return ctx.accum_read()

    first = nt.Batch(ctx, 4096, 8)
    handle = first._h.value
    assert_stats_equal(run(first, True), masked, "with qualities")
    first.release()
    again = nt.Batch(ctx, 3000, 8)   # rounded up to 3072 bytes: the pooled 4096 are within twice that
    assert again._h.value == handle
    assert_stats_equal(run(again, False), plain, "the pooled batch, without qualities")
    fresh = nt.Batch(ctx, 1 << 20, 64)
    assert fresh._h.value != handle
    assert_stats_equal(run(fresh, False), plain, "a fresh batch")
    again.release()
    fresh.release()
