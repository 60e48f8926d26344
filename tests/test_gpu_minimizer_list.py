"""The minimizer-list library (include/needletail_amd/minimizer_list.h, needletail_amd.MinimizerList) on a real MI355X, exact against
the host model (tests/_minimizer_list_model.py) and against the core's own windowed-minimizer digest.  The inputs are those of
tests/_minimizer_list_inputs.py, which tests/test_minimizer_list_model.py proves non-vacuous without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import _minimizer_list_inputs as I
import _minimizer_list_model as MM
import _stream_order as S
import needletail_amd as nt
import oracle as O  # the checker
from _count_helpers import pack, upload
from needletail_amd import _lib as NL
from needletail_amd import minimizer_lists as ML

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES, BITS, BITS_CANON = nt.PATH_BYTES_CANONICAL, nt.PATH_BITS, nt.PATH_BITS_CANONICAL
NONE, NORMALIZE = nt.PRE_NONE, nt.PRE_NORMALIZE
FOUR_PATHS = ((BYTES, NORMALIZE), (BITS, NONE), (BITS_CANON, NONE), (BITS_CANON, NORMALIZE))
ERR_BAD_ARG, ERR_CAPACITY = 2, 5
FIELDS = ("offsets", "pos", "values", "strand", "span")


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "these tests need a GPU"
    c = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
    c.close()


def dev_offsets(off):
    t = torch.from_numpy(np.asarray(off, dtype=np.uint64).view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def assert_csr(got, want, what):
    for name, g, w in zip(FIELDS, got, want):
        assert g.shape == np.asarray(w).shape and np.array_equal(g.astype(np.uint64), np.asarray(w).astype(np.uint64)), (what, name)


def listed(ml, dev, n_bytes, off, pre, **kw):
    ml.run_device(dev, n_bytes, dev_offsets(off), len(off) - 1, pre, **kw)
    return ml.read()


def digest_of(got, k):
    return MM.digest(got[2], got[3], got[4], k)


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- 1, 2: against the model ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 3])
def test_every_short_record(ctx, k):
    """Every record over ACGT of length 0..7 as one batch: every tie pattern of up to 7 - k + 1 keys, at w = 1..4, on the four paths,
    in both orders."""
    recs = I.short_records()
    buf, off = pack(recs), MM.packed_offsets(recs)
    dev = upload(buf)
    for w in (1, 2, 3, 4):
        for path, pre in FOUR_PATHS:
            for order in (ML.LEX, ML.HASH):
                with nt.MinimizerList(k, path, w, order, ctx) as ml:
                    got = listed(ml, dev, len(buf), off, pre)
                assert_csr(got, MM.csr(MM.entries_of(buf, k, w, path, pre, order), off, len(buf), k), (k, w, path, pre, order))


@pytest.mark.parametrize("k,w", I.KW)
def test_random_records_match_the_model(ctx, k, w):
    """Records of the lengths around k and k + w with N, lower case, U and IUPAC letters: every path with NORMALIZE and the bit paths
    with NONE, both orders, without and with a quality stream; the packer's route; then the empty inputs."""
    recs, quals = I.random_records(k, w)
    buf, off = pack(recs), MM.packed_offsets(recs)
    qual = np.frombuffer(b"".join(q + b"\xff" for q in quals), dtype=np.uint8)
    dev, dq = upload(buf), upload(qual.tobytes(), fill=0xFF)
    beyond = off.copy()
    beyond[-1] += 1000   # an offset beyond n_bytes reads as n_bytes
    for path, pre in ((BYTES, NORMALIZE), (BITS, NORMALIZE), (BITS_CANON, NORMALIZE), (BITS, NONE), (BITS_CANON, NONE)):
        for order in (ML.LEX, ML.HASH):
            with nt.MinimizerList(k, path, w, order, ctx) as ml:
                want = MM.csr(MM.entries_of(buf, k, w, path, pre, order), off, len(buf), k)
                got = listed(ml, dev, len(buf), off, pre)
                assert_csr(got, want, (k, w, path, pre, order))
                st = ml.stats()
                assert (st["k"], st["path"], st["w"], st["order"]) == (k, path, w, order)
                assert st["n_records"] == len(recs) and st["n_entries"] == want[1].size and st["n_windows"] == int(want[4].sum()) and st["n_chunks"] == 1
                assert np.all(want[4] >= 1) and np.all(want[4] <= w)
                assert_csr(listed(ml, dev, len(buf), beyond, pre), want, ("an offset beyond n_bytes", k, w, path, order))
                masked = MM.csr(MM.entries_of(buf, k, w, path, pre, order, qual, I.CUTOFF), off, len(buf), k)
                assert_csr(listed(ml, dev, len(buf), off, pre, d_qual=dq, quality_cutoff=I.CUTOFF), masked, ("quality", k, w, path, order))
                if order == ML.HASH and path == BYTES:   # the packer's route: the same records through ntk_batch_append, its offsets
                    ml.run_records(recs, pre)
                    assert_csr(ml.read(), want, ("run_records", k, w))
                    ml.run_records(recs, pre, quals, I.CUTOFF)
                    assert_csr(ml.read(), masked, ("run_records with qualities", k, w))
                    assert MM.lists(recs, k, w, path, pre, order, quals, I.CUTOFF)[1].tolist() == masked[1].tolist()
                    # the empty inputs: n_records empty ranges
                    ml.run_device(dev, 0, dev_offsets(off), len(recs), pre)
                    assert_csr(ml.read(), (np.zeros(len(recs) + 1), [], [], [], []), "n_bytes = 0")
                    ml.run_device(dev, len(buf), dev_offsets(off), 0, pre)
                    assert_csr(ml.read(), (np.zeros(1), [], [], [], []), "n_records = 0")
                    ml.run_records([], pre)
                    assert ml.read()[0].tolist() == [0] and ml.stats()["n_entries"] == 0 and ml.stats()["n_windows"] == 0
                    ml.run_records([b"", b"ACG"[: k - 1], b""], pre)
                    assert ml.read()[0].tolist() == [0, 0, 0, 0]


# ---- 3: against the core ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,w,route", [(21, 11, 0), (27, 7, NL.ROUTE_NO_REGFUSED), (21, 11, NL.ROUTE_TWO_PASS)])
def test_digest_is_the_cores(ctx, k, w, route):
    """On the same device batch, LEX order, the canonical paths: the list's digest is what ntk_minimizers_reduce_device folds - on the
    fused, the generic and the two-pass route - and what the oracle says."""
    host = O.synth_reads(0x5EED0031, 0, 3000, 150, 3)
    buf = host.tobytes()
    off = np.arange(3001, dtype=np.uint64) * 151
    dev = upload(buf)
    for path, pre, rule in ((BYTES, NORMALIZE, (True, True)), (BITS_CANON, NONE, (False, False))):
        ctx.set_option(NL.OPT_MINIMIZER_ROUTE, route)
        try:
            ctx.accum_reset()
            ctx.reduce_device(dev, len(buf), k, path, pre, w=w)
            core = ctx.accum_read()
        finally:
            ctx.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
        with nt.MinimizerList(k, path, w, ML.LEX, ctx) as ml:
            got = listed(ml, dev, len(buf), off, pre)
            mine = digest_of(got, k)
            assert ml.stats()["n_windows"] == core["n_total"]
        assert MM.same_digest(mine, core), (k, w, route, path)
        assert MM.same_digest(mine, O.minimizers_reduce(buf, k, w, *rule)), (k, w, path)
        assert got[0][-1] == got[1].size and mine["n_total"] > 0


# ---- 4, 6: tile seams and the capped grid -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", I.SEAM_W)
def test_tile_seams_of_the_select_kernel(ctx, w):
    """The all-A k-mer's first window end at every distance -(w + 1) .. w + 1 from a tile boundary, in the first, a middle and the last
    step of a block's loop (so the batch has more tiles than two steps of the capped grid of ml_select_kernel and ml_scatter_kernel):
    its entry has span w and neither splits nor doubles; and a record of one repeated base has an entry at every window, span 1."""
    k, grid = I.SEAM_K, n_cu() * MM.BLOCKS_PER_CU
    sp, aims = I.tile_seam_batch(w, grid)
    assert sp.n_bytes > 2 * grid * MM.TILE
    buf = sp.buf()
    with nt.MinimizerList(k, BITS, w, ML.LEX, ctx) as ml:
        got = listed(ml, upload(buf.tobytes()), sp.n_bytes, sp.offsets, NONE)
    want = sp.csr(k, w, BITS, NONE, ML.LEX)
    assert_csr(got, want, ("tile seams", w))
    offsets, pos, values, strand, span = got
    aimed = np.flatnonzero(values == 0)
    assert aimed.size == len(aims) == 3 * (2 * w + 3) and np.all(span[aimed] == w)
    starts = sp.offsets[:-1].astype(np.int64)
    rec = np.searchsorted(offsets, aimed, side="right") - 1
    assert np.array_equal(pos[aimed].astype(np.int64) + starts[rec] + k - 1, np.array(aims))   # the k-mer ends at its first window end
    last = slice(int(offsets[-2]), int(offsets[-1]))
    assert span[last].size == 3000 - (k + w - 1) + 1 and np.all(span[last] == 1) and np.all(np.diff(pos[last].astype(np.int64)) == 1)


def test_more_tiles_than_one_step_of_the_grid(ctx):
    """ML_BLOCKS_PER_CU blocks per compute unit is the cap of ml_select_kernel and ml_scatter_kernel (csrc/ntk_ml_rule.hpp): random
    reads over two and a half steps of it, against the oracle's digest and the record ranges."""
    k, w = 11, 5
    n_reads = int(2.5 * n_cu() * MM.BLOCKS_PER_CU * MM.TILE) // 151
    host = O.synth_reads(0x5EED0032, 0, n_reads, 150, 2)
    assert host.size > 2 * n_cu() * MM.BLOCKS_PER_CU * MM.TILE
    off = np.arange(n_reads + 1, dtype=np.uint64) * 151
    with nt.MinimizerList(k, BYTES, w, ML.LEX, ctx) as ml:
        got = listed(ml, upload(host.tobytes()), host.size, off, NORMALIZE)
    assert MM.same_digest(digest_of(got, k), O.minimizers_reduce(host, k, w, True, True))
    offsets, pos = got[0].astype(np.int64), got[1].astype(np.int64)
    assert offsets[0] == 0 and offsets[-1] == pos.size and np.all(np.diff(offsets) >= 0) and pos.max() <= 150 - k
    inside = np.ones(pos.size, dtype=bool)
    inside[offsets[1:-1][offsets[1:-1] < pos.size]] = False
    assert np.all(np.diff(pos)[inside[1:]] > 0)   # positions strictly increase inside a record


@pytest.mark.parametrize("k,w,order,path,pre", I.GRID_CASES)
def test_exact_past_one_step_of_the_grid(ctx, k, w, order, path, pre):
    """Random 150-base reads over 1.25 steps of the capped grid of ml_select_kernel and ml_scatter_kernel, with the quality stream: every
    field of every entry against the model - random content, ties, N and masked bases at every tile boundary, blocks of the scatter kernel
    that walk the record starts along a run of two tiles."""
    grid = n_cu() * MM.BLOCKS_PER_CU
    buf, qual, off = I.grid_batch(grid)
    assert len(buf) > grid * MM.TILE
    want = MM.csr(MM.entries_of(buf, k, w, path, pre, order, qual, I.CUTOFF), off, len(buf), k)
    with nt.MinimizerList(k, path, w, order, ctx) as ml:
        got = listed(ml, upload(buf), len(buf), off, pre, d_qual=upload(qual.tobytes(), fill=0xFF), quality_cutoff=I.CUTOFF)
        st = ml.stats()
    assert_csr(got, want, ("exact past one step", k, w, order, path))
    assert st["n_entries"] == want[1].size > grid and st["n_windows"] == int(want[4].sum()) and st["n_chunks"] == 1


def test_record_starts_carried_along_a_blocks_tiles(ctx):
    """2.25 steps of the capped grid, so a block of ml_scatter_kernel takes three consecutive tiles and carries the record starts it
    knows from one to the next: 5 000 equal starts inside a tile with entries in front of a tile with entries; a tile without entries
    that holds 5 000 equal starts, skipped between two tiles with entries of the same block; and two skipped tiles in front of a block's
    only tile with entries, far into the starts.  Exact, both orders."""
    k, w = I.CARRY_KW
    grid = n_cu() * MM.BLOCKS_PER_CU
    sp, _ = I.carry_batch(grid)
    assert -(-(sp.n_bytes // MM.TILE) // grid) == 3
    dev = upload(sp.buf().tobytes())
    for order in (ML.LEX, ML.HASH):
        with nt.MinimizerList(k, BITS, w, order, ctx) as ml:
            got = listed(ml, dev, sp.n_bytes, sp.offsets, NONE)
            assert ml.stats()["n_chunks"] == 1
        assert_csr(got, sp.csr(k, w, BITS, NONE, order), ("carried record starts", order))
        assert got[1].size > 1000 and int(got[1].max()) <= 200 - k


# ---- the offsets the header defines, the two other pre-steps ---------------------------------------------------------------------------------

def test_offsets_that_are_not_the_packers(ctx):
    """The header's sentence on offsets that are not the packer's: offsets[0] > 0, offsets[n_records] < n_bytes, runs of 5 000 equal
    starts in the middle of a tile with entries and in a stretch of tiles without any, and 36 equal starts in front of the last one (the
    doubling search of a tile's starts steps over offsets[n_records]).  offsets_out and pos are the header's, entries outside every
    record's range included.  Six tiles: every block of ml_scatter_kernel has one tile and searches the starts from the first on; the
    starts a block carries from tile to tile are test_record_starts_carried_along_a_blocks_tiles'."""
    k, w = I.ODD_KW
    buf, off = I.odd_offsets_batch()
    dev = upload(buf)
    for order in (ML.LEX, ML.HASH):
        want = MM.csr(MM.entries_of(buf, k, w, BITS, NONE, order), off, len(buf), k)
        with nt.MinimizerList(k, BITS, w, order, ctx) as ml:
            got = listed(ml, dev, len(buf), off, NONE)
            assert ml.stats()["n_records"] == off.size - 1 > 2 * I.ODD_RUN
        assert_csr(got, want, ("odd offsets", order))
        assert got[0][0] > 0 and got[0][-1] < got[1].size


@pytest.mark.parametrize("path,pre", I.IUPAC_PATH_PRES)
def test_strip_returns_and_normalize_iupac(ctx, path, pre):
    """The two pre-steps no other case of this file passes, on records with IUPAC letters of either case, U and u."""
    k, w = I.IUPAC_KW
    recs = I.iupac_records()
    buf, off = pack(recs), MM.packed_offsets(recs)
    dev = upload(buf)
    for order in (ML.LEX, ML.HASH):
        with nt.MinimizerList(k, path, w, order, ctx) as ml:
            got = listed(ml, dev, len(buf), off, pre)
        assert_csr(got, MM.lists(recs, k, w, path, pre, order), ("pre-step", path, pre, order))
        assert got[1].size > 100


# ---- 5, 7: the chunk seam and the held list ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def chunk_batch():
    """64 MiB + 8 KiB of N on the device, uploaded once; a case rewrites its region."""
    t = torch.full((I.CHUNK_BYTES + 64,), ord("N"), dtype=torch.uint8, device="cuda")
    off = dev_offsets([0, I.CHUNK_BYTES])
    yield t, off
    del t
    torch.cuda.empty_cache()


def _place(dev, sp, lo, hi):
    """The bytes [lo, hi) of the case onto the device batch."""
    dev[lo:hi] = torch.from_numpy(sp.region(lo, hi)).cuda()


@pytest.mark.parametrize("k,w", I.CHUNK_KW)
def test_chunk_seam(ctx, chunk_batch, k, w):
    """The aimed k-mer's first window end at seam + d for every d in -(w + k) .. w + k: on both sides of the seam, its windows split
    between the chunks at every s of w = s + (w - s), the k-mer itself across the seam; exact against the model, span w every time."""
    dev, d_off = chunk_batch
    lo, hi = I.chunk_seam_region(k, w)
    _place(dev, I.chunk_seam_case(k, w, 0)[0], 0, 2 * I.EARLY_AT)   # the early piece is every case's
    _place(dev, I.chunk_seam_case(k, w, 0)[0], I.CHUNK_BYTES - 16, I.CHUNK_BYTES)   # ... and the break byte
    with nt.MinimizerList(k, BITS, w, ML.LEX, ctx) as ml:
        for d in I.chunk_seam_ds(k, w):
            sp, e = I.chunk_seam_case(k, w, d)
            _place(dev, sp, lo, hi)
            ml.run_device(dev, I.CHUNK_BYTES, d_off, 1, NONE)
            got = ml.read()
            assert_csr(got, sp.csr(k, w, BITS, NONE, ML.LEX), ("chunk seam", k, w, d))
            aimed = np.flatnonzero(got[2] == 0)
            assert aimed.size == 1 and got[4][aimed[0]] == w and int(got[1][aimed[0]]) + k - 1 == e, d
            assert ml.stats()["n_chunks"] == 2
    dev[lo:hi] = ord("N")


@pytest.mark.parametrize("k,w", I.CHUNK_KW)
def test_many_records_around_the_chunk_seam(ctx, chunk_batch, k, w):
    """Thousands of packed records of 0 .. 300 bases around the seam, in HASH order: the second chunk's blocks of ml_scatter_kernel find
    their record among all the starts of the first chunk; a record that straddles the seam, a start inside the halo, and starts exactly at
    the seam and one byte to either side."""
    dev, _ = chunk_batch
    with nt.MinimizerList(k, BITS, w, ML.HASH, ctx) as ml:
        for layout in I.SEAM_LAYOUTS:
            sr = I.seam_records(k, w, layout)
            for lo, hi in ((0, 2 * I.EARLY_AT), (I.SEAM_LO - 16, I.SEAM_HI + 16), (I.CHUNK_BYTES - 16, I.CHUNK_BYTES)):
                _place(dev, sr, lo, hi)
            n_records = sr.offsets.size - 1
            ml.run_device(dev, I.CHUNK_BYTES, dev_offsets(sr.offsets), n_records, NONE)
            assert_csr(ml.read(), sr.csr(k, w, BITS, NONE, ML.HASH), ("many records at the chunk seam", k, w, layout))
            st = ml.stats()
            assert st["n_chunks"] == 2 and st["n_records"] == n_records >= 2000
    dev[I.SEAM_LO - 16: I.SEAM_HI + 16] = ord("N")


def test_held_list(ctx, chunk_batch):
    """Growth keeps the prefix (the second chunk adds more entries than the first allocation holds), a smaller run replaces the result,
    read with a capacity too small, exact and NULL, trim, device_bytes against the header's statement, two runs alike."""
    k, w = 32, 256
    dev, d_off = chunk_batch
    sp, (lo, hi) = I.growth_case(k, w)
    for a, b in ((lo, hi), (0, 2 * I.EARLY_AT), (I.CHUNK_BYTES - 16, I.CHUNK_BYTES)):
        _place(dev, sp, a, b)
    ent = sp.entries(k, w, BITS, NONE, ML.HASH)
    per_chunk = [int((ent.end < MM.CHUNK).sum()), int((ent.end >= MM.CHUNK).sum())]
    assert per_chunk[0] > 0 and per_chunk[0] + per_chunk[1] > MM.grow_half_again(per_chunk[0]), "the second chunk outgrows the first allocation"
    want = sp.csr(k, w, BITS, NONE, ML.HASH)
    lib = ML.lib()
    with nt.MinimizerList(k, BITS, w, ML.HASH, ctx) as ml:
        n = C.c_uint64(7)
        assert lib.ntk_minimizer_list_read(ml._h, None, None, None, None, 0, C.byref(n)) == 0 and n.value == 0   # before any run
        assert ml.stats()["device_bytes"] == 0 and ml.device_arrays() == (0, 0, 0, 0, 0)
        ml.run_device(dev, I.CHUNK_BYTES, d_off, 1, NONE)
        got = ml.read()
        assert_csr(got, want, "growth keeps the prefix")
        assert ml.stats()["device_bytes"] == MM.device_bytes(I.CHUNK_BYTES, 1, k, w, per_chunk)
        ml.run_device(dev, I.CHUNK_BYTES, d_off, 1, NONE)
        assert_csr(ml.read(), got, "two runs alike")
        # the capacity protocol
        total = want[1].size
        offsets = np.full(2, 77, dtype=np.uint64)
        pos, values, info = (np.full(total, 77, dtype=t) for t in (np.uint64, np.uint64, np.uint32))
        p = lambda x: x.ctypes.data   # noqa: E731
        assert lib.ntk_minimizer_list_read(ml._h, None, None, None, None, 0, C.byref(n)) == ERR_CAPACITY and n.value == total
        assert lib.ntk_minimizer_list_read(ml._h, p(offsets), p(pos), p(values), p(info), total - 1, C.byref(n)) == ERR_CAPACITY and n.value == total
        assert offsets.tolist() == [77, 77] and np.all(pos == 77) and np.all(values == 77) and np.all(info == 77), "nothing is written"
        assert lib.ntk_minimizer_list_read(ml._h, None, p(pos), p(values), p(info), total, C.byref(n)) == 0 and np.all(pos == 77)
        assert lib.ntk_minimizer_list_read(ml._h, p(offsets), p(pos), p(values), p(info), total, C.byref(n)) == 0
        assert np.array_equal(pos, want[1]) and np.array_equal(info >> 1, want[4]) and offsets.tolist() == [0, total]
        assert lib.ntk_minimizer_list_read(ml._h, p(offsets), None, None, None, total, C.byref(n)) == ERR_BAD_ARG
        # a smaller run replaces the result
        small = [b"T" * 400, b"", b"ACGT" * 80]
        ml.run_records(small, NONE)
        assert_csr(ml.read(), MM.lists(small, k, w, BITS, NONE, ML.HASH), "a smaller run")
        ml.trim()
        assert ml.stats()["device_bytes"] == 0 and ml.stats()["n_records"] == 0 and ml.read()[1].size == 0
        assert lib.ntk_minimizer_list_read(ml._h, None, None, None, None, 0, C.byref(n)) == 0 and n.value == 0
        sbuf = pack(small)
        ml.run_device(upload(sbuf), len(sbuf), dev_offsets(MM.packed_offsets(small)), 3, NONE)
        n_small = MM.lists(small, k, w, BITS, NONE, ML.HASH)[1].size
        assert ml.stats()["device_bytes"] == MM.device_bytes(len(sbuf), 3, k, w, [n_small]) and n_small > 0
    dev[lo:hi] = ord("N")


# ---- 8: the result on the device ----------------------------------------------------------------------------------------------------------

class _DeviceView:
    def __init__(self, address, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (address, False), "version": 2}


def test_result_device_is_what_read_returns(ctx):
    recs, _ = I.random_records(21, 11)
    with nt.MinimizerList(21, BYTES, 11, ML.HASH, ctx) as ml:
        ml.run_records(recs, NORMALIZE)
        offsets, pos, values, strand, span = ml.read()
        d_off, d_pos, d_val, d_info, n = ml.device_arrays()
        assert n == pos.size > 0 and all((d_off, d_pos, d_val, d_info))
        clone = lambda a, m, t: torch.as_tensor(_DeviceView(a, m, t), device="cuda").clone().cpu().numpy()   # noqa: E731
        assert np.array_equal(clone(d_off, len(recs) + 1, "<i8").view(np.uint64), offsets)
        assert np.array_equal(clone(d_pos, n, "<i8").view(np.uint64), pos) and np.array_equal(clone(d_val, n, "<i8").view(np.uint64), values)
        info = clone(d_info, n, "<i4").view(np.uint32)
        assert np.array_equal(info & 1, strand) and np.array_equal(info >> 1, span)
        assert ml.device_arrays() == (d_off, d_pos, d_val, d_info, n)   # the pointers stay until the next run


# ---- 9: stream order ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available(), "these tests need a GPU"
    S.cycles_per_ms()
    r = S.Rig()
    yield r
    r.close()


def test_stream_order(rig):
    """ntk_minimizer_list_run_device behind a spin: the batch, the quality stream and the offsets are produced behind the hold (the decoy
    in front), the inputs clobbered behind the call; read, stats and result_device are made with that work pending.  run_device, read,
    stats and trim are SYNC; result_device queues nothing and waits for nothing."""
    k, w = 21, 11
    t, d = I.stream_batches()
    want = MM.csr(MM.entries_of(t.buf, k, w, BYTES, NORMALIZE, ML.HASH, t.qual, S.CUTOFF), t.offsets, t.n, k)
    seq = S.batch_input(t.buf, d.buf)
    qual = S.Input(S.dev_bytes(t.qual.tobytes(), fill=0xFF), S.dev_bytes(d.qual.tobytes(), fill=0xFF), 0)
    off = S.words_input(t.offsets, np.zeros_like(t.offsets), 0)
    with nt.MinimizerList(k, BYTES, w, ML.HASH, rig.ctx) as ml:
        def call():
            ml.run_device(seq.buf, t.n, off.buf, S.N_RECORDS, NORMALIZE, d_qual=qual.buf, quality_cutoff=S.CUTOFF)

        def read():
            arrays = ml.device_arrays()
            return ml.read(), ml.stats(), arrays

        for plain in (True, False):
            _, _, (got, st, arrays) = S.hazard_call(rig, S.SYNC, [seq, qual, off], [], call, read, plain=plain)
            assert_csr(got, want, ("stream order", plain))
            assert st["n_entries"] == want[1].size == arrays[4] and st["n_windows"] == int(want[4].sum())
        S.hazard_call(rig, S.SYNC, [], [], ml.read)
        S.hazard_call(rig, S.SYNC, [], [], ml.stats)
        _, _, _ = S.hazard_call(rig, S.ASYNC, [], [], ml.device_arrays)   # with the hold pending: it returns before the stream drains
        # trim frees every array: with a hold pending it has to wait for the stream first, and the result is gone after it
        S.hazard_call(rig, S.SYNC, [], [], ml.trim)
        assert ml.stats()["n_entries"] == 0 and ml.read()[1].size == 0


# ---- 10: the example program ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args,order", [((), MM.LEX), (("-k", "15", "-w", "10", "-H"), MM.HASH)])
def test_example_program_on_the_golden_28s(args, order):
    exe, path = os.path.join(ROOT, "examples", "minimizers"), os.path.join(ROOT, "tests", "golden", "28S.fasta")
    k = int(args[1]) if args else 21
    w = int(args[3]) if args else 11
    names, recs = [], []
    for line in open(path, "rb").read().splitlines():
        if line.startswith(b">"):
            names.append(line[1:].split()[0].decode() if line[1:].split() else "")
            recs.append(b"")
        elif recs:
            recs[-1] += line.strip()
    offsets, pos, values, strand, span = MM.lists(recs, k, w, BYTES, NORMALIZE, order)
    want = [f"{names[r]}\t{int(pos[i])}\t{'-' if strand[i] else '+'}\t{O.bitmer_to_bytes(int(values[i]), k).decode()}\t{int(span[i])}"
            for r in range(len(recs)) for i in range(int(offsets[r]), int(offsets[r + 1]))]
    r = subprocess.run([exe, *args, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert len(want) > 100 and r.stdout.splitlines() == want
