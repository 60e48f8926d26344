"""The seed-index library (include_staged/needletail_amd/seed_index.h, needletail_amd.SeedIndex) on a real MI355X, exact against the
host model (tests/_seed_index_model.py), field by field: a_offsets, ref, rev, rpos, qpos, rows and the stats.  The inputs are those of
tests/_seed_index_inputs.py, which tests/test_seed_index_inputs.py proves non-vacuous without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import _minimizer_list_model as MM
import _seed_index_inputs as I
import _seed_index_model as M
import _stream_order as S
import needletail_amd as nt
from needletail_amd import seeding as SD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTES, BITS_CANON, NORMALIZE = nt.PATH_BYTES_CANONICAL, nt.PATH_BITS_CANONICAL, nt.PRE_NORMALIZE


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "these tests need a GPU"
    c = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev_list(lst):
    """The list as four device tensors (int64 for the 8-byte words, int32 for info), exactly as long as the list."""
    off, pos, values, info = lst
    words = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()   # noqa: E731
    out = (words(off), words(pos), words(values), torch.from_numpy(np.ascontiguousarray(info, dtype=np.uint32).view(np.int32).copy()).cuda())
    torch.cuda.synchronize()
    return out


def assert_result(got, want, what):
    for name, g, w in zip(M.FIELDS, got, want):
        assert g.shape == np.asarray(w).shape and np.array_equal(g.astype(np.uint64), np.asarray(w).astype(np.uint64)), (what, name)


def assert_stats(si, index, lst=None, n_anchors=0, what=None):
    st = si.stats()
    assert {k: v for k, v in st.items() if k != "device_bytes"} == M.stats(index, lst, n_anchors), what
    assert list(st) == list(M.STATS)
    return st


def matched(si, index, lst, max_occ=0, what=None, dev=None):
    """Match `lst` (uploaded, or the tensors `dev`) and hold the whole result and the stats to the model."""
    si.match(dev_list(lst) if dev is None else dev, max_occ)
    status, want, total = M.match(index, lst, max_occ)
    assert status == M.OK
    got = si.read()
    assert_result(got, want, (what, max_occ))
    assert_stats(si, index, lst, total, (what, max_occ))
    return got


def status_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except nt.NtkError as e:
        return e.status
    return M.OK


# ---- fabricated lists -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("front,back", [(0, 0), (3, 2)])
def test_small_lists_under_every_max_occ(ctx, front, back):
    """3 references and 8 reads of at most 12 entries, every max_occ 0..4; then the same lists with entries in front of offsets[0] and
    behind offsets[n] that belong to no record - a pos of 2^32 among them, which nothing looks at."""
    refs, reads = I.small_case(front, back)
    index = M.Index(refs)
    with nt.SeedIndex(ctx) as si:
        si.build(dev_list(refs))
        assert_stats(si, index)
        d_reads = dev_list(reads)
        for max_occ in range(5):
            got = matched(si, index, reads, max_occ, "small", d_reads)
            assert np.array_equal(got[5][:, 0], got[5][:, 1:].sum(axis=1))
        assert np.array_equal(si.spectrum(8), index.spectrum(8)) and np.array_equal(si.spectrum(2), index.spectrum(2))


@pytest.mark.parametrize("seed", I.RANDOM_SEEDS)
def test_random_lists_match_the_model(ctx, seed):
    refs, reads = I.random_case(seed)
    index = M.Index(refs)
    with nt.SeedIndex(ctx) as si:
        si.build(dev_list(refs))
        for max_occ in (0, 1, I.RANDOM_MAX_OCC, 100):
            matched(si, index, reads, max_occ, ("random", seed))
        for n_bins in (2, 3, index.max_occ, index.max_occ + 1, index.max_occ + 2, 5000):
            assert np.array_equal(si.spectrum(n_bins), index.spectrum(n_bins)), n_bins
        for ppm in (0, 200, 50_000, 100_000, 500_000, 1_000_000):
            assert si.occ_cutoff(ppm) == index.occ_cutoff(ppm), ppm


def test_empty_inputs_and_match_before_build(ctx):
    refs, reads = I.small_case()
    with nt.SeedIndex(ctx) as si:
        assert status_of(si.match, dev_list(reads)) == M.ERR_BAD_ARG, "match before any build"
        assert si.read()[1].size == 0 and si.stats()["n_reads"] == 0 and si.device_arrays()[:5] == (0, 0, 0, 0, 0)
        assert status_of(si.spectrum, 8) == M.ERR_BAD_ARG
        for r in (I.empty_list(0), I.empty_list(3)):   # an empty index: no references, references without entries
            si.build(dev_list(r))
            index = M.Index(r)
            assert_stats(si, index)
            assert not si.spectrum(4).any() and si.occ_cutoff(200) == 1
            got = matched(si, index, reads, 2, "empty index")
            assert got[1].size == 0 and np.array_equal(got[5][:, 3], got[5][:, 0])
        si.build(dev_list(refs))
        index = M.Index(refs)
        for q in (I.empty_list(0), I.empty_list(4)):   # n_reads = 0; reads without seeds
            got = matched(si, index, q, 0, "empty reads")
            assert got[0].size == q[0].size and not got[0].any()


def test_refusals_leave_the_held_result_unchanged(ctx):
    """Offsets decreasing, offsets[n] > n and a pos of 2^32 - in a build and in a match: the index and the held match are what they
    were.  Then the refusals that come before any device call."""
    refs, reads = I.small_case()
    index = M.Index(refs)
    with nt.SeedIndex(ctx) as si:
        si.build(dev_list(refs))
        before = matched(si, index, reads, 2, "before")
        arrays, st = si.device_arrays(), si.stats()
        for what, lst, status in I.refused_lists():
            assert M.verify(lst) == status
            d = dev_list(lst)
            assert status_of(si.match, d, 2) == status, what
            assert status_of(si.build, d) == status, what
            assert_result(si.read(), before, what)
            assert si.device_arrays() == arrays and si.stats() == st, what
        matched(si, index, reads, 0, "after")   # the index is intact
        d = dev_list(reads)
        lib, h = SD.lib(), si._h
        p = [C.c_void_p(t.data_ptr()) for t in d]
        n_reads, n = reads[0].size - 1, reads[1].size
        for call in (lambda *a: lib.ntk_seed_index_build_device(h, *a), lambda *a: lib.ntk_seed_index_match_device(h, *a, 0, 0)):
            assert call(p[0], p[1], p[2], p[3], n_reads, 1 << 32) == M.ERR_BAD_ARG and call(p[0], p[1], p[2], p[3], 1 << 31, n) == M.ERR_BAD_ARG
            assert call(None, p[1], p[2], p[3], n_reads, n) == M.ERR_BAD_ARG and call(p[0], None, p[2], p[3], n_reads, n) == M.ERR_BAD_ARG
            assert call(C.c_void_p(p[0].value + 4), p[1], p[2], p[3], n_reads, n) == M.ERR_BAD_ARG
            assert call(p[0], p[1], p[2], C.c_void_p(p[3].value + 2), n_reads, n) == M.ERR_BAD_ARG
        matched(si, index, reads, 0, "after the host-side refusals", d)


# ---- the two sort routes, the balanced fill, the capped grids ---------------------------------------------------------------------------

@pytest.mark.parametrize("n_anchors", [SD.SORT_TILE - 1, SD.SORT_TILE, SD.SORT_TILE + 1, 3 * SD.SORT_TILE + 5])
def test_both_sort_routes_around_the_tile(ctx, n_anchors):
    """One read with exactly n_anchors anchors between short reads: in LDS up to SORT_TILE, through the segmented sorts beyond.  The
    fill's order is not the sorted one, every (ref_rev, rpos) is there under two qpos, and the later qpos comes first in the list."""
    assert SD.SORT_TILE == M.SORT_TILE
    refs, reads = I.sort_route_case(n_anchors)
    index = M.Index(refs)
    with nt.SeedIndex(ctx) as si:
        si.build(dev_list(refs))
        got = matched(si, index, reads, 0, ("sort route", n_anchors))
        assert int(got[0][4] - got[0][3]) == n_anchors
        # the arrays of the long route hold the long read's anchors alone, and are there only where a read is long
        long_anchors = M.long_anchors(got[0])
        assert long_anchors == (n_anchors if n_anchors > SD.SORT_TILE else 0)
        assert si.stats()["device_bytes"] == M.device_bytes(index.n_keys, index.n_entries, n_reads=7, n_seeds=reads[1].size,
                                                            n_anchors=n_anchors + 6, long_anchors=long_anchors)
        matched(si, index, reads, 2, ("sort route, the long read repetitive", n_anchors))


def test_one_seed_with_20000_occurrences_among_seeds_with_one(ctx):
    """The balanced fill; the long read lies more than 2.25 steps of a block per read into the batch (si_widen_kernel, si_narrow_kernel
    and si_sort_kernel loop)."""
    refs, reads = I.balanced_fill_case(n_cu())
    index = M.Index(refs)
    with nt.SeedIndex(ctx) as si:
        si.build(dev_list(refs))
        d = dev_list(reads)
        got = matched(si, index, reads, 0, "balanced fill", d)
        assert int(np.diff(got[0].astype(np.int64)).max()) == 20_002
        matched(si, index, reads, 20_000, "occ == max_occ is kept", d)
        assert matched(si, index, reads, 19_999, "occ == max_occ + 1 is not", d)[1].size == reads[0].size


@pytest.mark.parametrize("quarters", [5, 9])
def test_more_items_than_one_step_of_every_capped_grid(ctx, quarters):
    """1.25 and 2.25 steps of entries (the build's kernels) and of seeds and anchors (the match's), worked out from the device's CU
    count and the rule header's factors; at most one occurrence per seed."""
    refs, reads = I.capped_grid_case(n_cu(), quarters)
    step = n_cu() * M.BLOCKS_PER_CU * M.THREADS
    index = M.Index(refs)
    assert index.n_entries > quarters * step // 4 and reads[1].size > quarters * step // 4
    with nt.SeedIndex(ctx) as si:
        si.build(dev_list(refs))
        assert_stats(si, index)
        assert np.array_equal(si.spectrum(4), index.spectrum(4))
        got = matched(si, index, reads, 1, ("capped grids", quarters))
        assert got[1].size > (quarters - 1) * step // 4


def test_max_anchors_one_below_the_total_and_the_exact_total(ctx):
    refs, reads = I.small_case()
    index = M.Index(refs)
    _, full, total = M.match(index, reads, 0)
    with nt.SeedIndex(ctx) as si:
        si.build(dev_list(refs))
        d = dev_list(reads)
        si.match(d, 0, max_anchors=total)
        assert_result(si.read(), full, "the exact total")
        assert status_of(si.match, d, 0, max_anchors=total - 1) == M.ERR_CAPACITY
        status, want, needed = M.match(index, reads, 0, max_anchors=total - 1)
        assert status == M.ERR_CAPACITY and needed == total
        assert_result(si.read(), want, "one below the total: the rows are valid and no anchor is held")
        assert_stats(si, index, reads, total, "n_anchors is the number needed")
        assert si.device_arrays()[5] == 0
        assert status_of(si.match, d, 0, max_anchors=1) == M.ERR_CAPACITY
        matched(si, index, reads, 4, "after the refusal", d)


# ---- end to end through the minimizer lists -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,w,order,path", I.END_TO_END)
def test_reads_cut_from_references_lie_on_their_diagonals(ctx, k, w, order, path):
    """3 random references of 2 kb, 60 reads of 150 bp cut from them forward and reverse-complemented, some random: the lists go from
    MinimizerList to SeedIndex on the device; the result is the model's on the lists read back, and every anchor of a cut read on its
    own reference lies on the diagonal of its cut."""
    refs, reads, cuts = I.sequences()
    with nt.MinimizerList(k, path, w, order, ctx) as r_ml, nt.MinimizerList(k, path, w, order, ctx) as q_ml, nt.SeedIndex(ctx) as si:
        r_ml.run_records(refs, NORMALIZE)
        q_ml.run_records(reads, NORMALIZE)
        si.build(r_ml)
        si.match(q_ml)
        got = si.read()
        r_list, q_list = I.as_seed_list(r_ml.read()), I.as_seed_list(q_ml.read())
        index = M.Index(r_list)
        status, want, total = M.match(index, q_list, 0)
        assert_result(got, want, "end to end")
        assert_stats(si, index, q_list, total)
        cutoff = si.occ_cutoff(200)
        assert cutoff == index.occ_cutoff(200)
        si.match(q_ml, max_occ=cutoff)
        assert_result(si.read(), M.match(index, q_list, cutoff)[1], "under the cutoff")
    for a, b in zip(r_list, I.as_seed_list(MM.lists(refs, k, w, path, NORMALIZE, order))):
        assert np.array_equal(a, b)
    off, on = I.diagonal_exceptions(got, cuts, k)
    assert off == [] and on > 400


# ---- held state -------------------------------------------------------------------------------------------------------------------------------

class _DeviceView:
    def __init__(self, address, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (address, False), "version": 2}


def test_held_state(ctx):
    """A second match replaces the first; trim keeps the index; a build drops the held match; result_device is what read returns;
    device_bytes is the model's."""
    refs, reads = I.small_case()
    other_refs, other_reads = I.random_case(I.RANDOM_SEEDS[0])
    index = M.Index(refs)
    with nt.SeedIndex(ctx) as si:
        si.build(dev_list(refs))
        assert si.stats()["device_bytes"] == M.device_bytes(index.n_keys, index.n_entries), "rocPRIM's temporary storage is not held"
        matched(si, index, other_reads, 0, "first")
        first = matched(si, index, reads, 2, "second")
        # result_device is what read returns
        d_a_offsets, d_ref_rev, d_rpos, d_qpos, d_rows, n = si.device_arrays()
        assert n == first[1].size and all((d_a_offsets, d_ref_rev, d_rpos, d_qpos, d_rows))
        clone = lambda a, m, t: torch.as_tensor(_DeviceView(a, m, t), device="cuda").clone().cpu().numpy()   # noqa: E731
        assert np.array_equal(clone(d_a_offsets, first[0].size, "<i8").view(np.uint64), first[0])
        assert np.array_equal(clone(d_ref_rev, n, "<i4").view(np.uint32), first[1] << 1 | first[2])
        assert np.array_equal(clone(d_rpos, n, "<i4").view(np.uint32), first[3]) and np.array_equal(clone(d_qpos, n, "<i4").view(np.uint32), first[4])
        assert np.array_equal(clone(d_rows, first[5].size, "<i4").view(np.uint32), first[5].reshape(-1))
        assert si.device_arrays() == (d_a_offsets, d_ref_rev, d_rpos, d_qpos, d_rows, n)   # the pointers stay until the next match
        # trim frees the match and the work arrays, and the index stays: its bytes are the header's, and it matches again
        si.trim()
        st = assert_stats(si, index)
        assert st["device_bytes"] == M.index_bytes(index.n_keys, index.n_entries)
        assert si.read()[1].size == 0 and si.device_arrays() == (0, 0, 0, 0, 0, 0)
        assert_result(matched(si, index, reads, 2, "after trim"), first, "after trim")
        st = si.stats()
        total = first[1].size
        # the build's work arrays are gone, the match's are back
        assert st["device_bytes"] == M.device_bytes(index.n_keys, index.n_entries, n_reads=8, n_seeds=reads[1].size, n_anchors=total, build_work=False)
        # a build drops the held match
        si.build(dev_list(other_refs))
        other = M.Index(other_refs)
        assert_stats(si, other)
        assert si.read()[1].size == 0 and si.device_arrays()[5] == 0
        matched(si, other, other_reads, I.RANDOM_MAX_OCC, "against the new index")
        # the index arrays are those of the index held: a larger one before it leaves nothing behind
        assert other.n_entries > index.n_entries and other.n_keys > index.n_keys
        si.trim()
        assert si.stats()["device_bytes"] == M.index_bytes(other.n_keys, other.n_entries)
        si.build(dev_list(refs))
        si.trim()
        assert assert_stats(si, index)["device_bytes"] == M.index_bytes(index.n_keys, index.n_entries)
        matched(si, index, reads, 2, "against the smaller index")
        with pytest.raises(ValueError):
            si.match(dev_list(reads), 1 << 32)
        with pytest.raises(ValueError):
            si.match(dev_list(reads), 0, max_anchors=-1)
    with nt.SeedIndex(ctx) as a, nt.SeedIndex(ctx) as b:   # the same calls hold the same memory
        for si in (a, b):
            si.build(dev_list(refs))
            si.match(dev_list(reads), 2)
            si.spectrum(7)
        assert a.stats() == b.stats()
        assert a.stats()["device_bytes"] == M.device_bytes(index.n_keys, index.n_entries, n_reads=8, n_seeds=reads[1].size, n_anchors=first[1].size, n_bins=7)


# ---- the stream contract ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available(), "these tests need a GPU"
    S.cycles_per_ms()
    r = S.Rig()
    yield r
    r.close()


def list_inputs(true, decoy):
    """The four arrays of a list as hazard inputs: the decoy is in them when the call is made, the true list is copied over it behind
    the hold, and zeros - an empty list - are written over it behind the call."""
    t, d = dev_list(true), dev_list(decoy)
    return [S.Input(a, b, 0) for a, b in zip(t, d)]


def test_stream_order(rig):
    """Every call with work pending on the context's stream: the lists are produced behind the hold (a decoy of the same shape in front)
    and clobbered behind the call; read, stats and device_arrays are made with that work pending.  build_device, spectrum, match_device,
    read, stats and trim are SYNC; result_device queues nothing and waits for nothing."""
    refs, reads = I.small_case()
    index = M.Index(refs)
    decoy = lambda lst: (lst[0], lst[1] + np.uint64(1), lst[2] ^ np.uint64(0x10), lst[3] ^ np.uint32(1))   # noqa: E731
    r_in, q_in = list_inputs(refs, decoy(refs)), list_inputs(reads, decoy(reads))
    status, want, total = M.match(index, reads, 2)
    assert any(not np.array_equal(a, b) for a, b in zip(want, M.match(M.Index(decoy(refs)), reads, 2)[1])), "the decoy index is another one"
    with nt.SeedIndex(rig.ctx) as si:
        def build():
            si.build(tuple(i.buf for i in r_in))

        def match():
            si.match(tuple(i.buf for i in q_in), 2)

        def read():
            arrays = si.device_arrays()
            return si.read(), si.stats(), arrays

        for plain in (True, False):
            S.hazard_call(rig, S.SYNC, r_in, [], build, si.stats, plain=plain)
            assert np.array_equal(S.hazard_call(rig, S.SYNC, [], [], lambda: si.spectrum(8))[0], index.spectrum(8))
            _, _, (got, st, arrays) = S.hazard_call(rig, S.SYNC, q_in, [], match, read, plain=plain)
            assert_result(got, want, ("stream order", plain))
            assert st["n_anchors"] == total == arrays[5] and st["n_keys"] == index.n_keys
        S.hazard_call(rig, S.SYNC, [], [], si.read)
        S.hazard_call(rig, S.SYNC, [], [], si.stats)
        S.hazard_call(rig, S.ASYNC, [], [], si.device_arrays)   # with the hold pending: it returns before the stream drains
        # trim frees the match: with a hold pending it has to wait for the stream first; the index stays
        S.hazard_call(rig, S.SYNC, [], [], si.trim)
        assert si.stats()["n_keys"] == index.n_keys and si.read()[1].size == 0


# ---- the example program ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args,order,max_occ", [(("-a",), MM.HASH, 0), (("-k", "21", "-w", "11", "-o", "lex", "-f", "2", "-a"), MM.LEX, 2),
                                                (("-f", "1"), MM.HASH, 1)])
def test_example_program_on_the_golden_28s(tmp_path, args, order, max_occ):
    exe, path = os.path.join(ROOT, "examples", "seed_reads"), os.path.join(ROOT, "tests", "golden", "28S.fasta")
    k = int(args[1]) if "-k" in args else 15
    w = int(args[3]) if "-w" in args else 10
    names, recs = [], []
    for line in open(path, "rb").read().splitlines():
        if line.startswith(b">"):
            names.append(line[1:].split()[0].decode() if line[1:].split() else "")
            recs.append(b"")
        elif recs:
            recs[-1] += line.strip()
    rng = np.random.default_rng(0x285)
    reads = []
    for q in range(40):
        r = int(rng.integers(0, len(recs)))
        s = int(rng.integers(0, max(1, len(recs[r]) - 200)))
        piece = recs[r][s: s + 200].upper()
        reads.append(I.revcomp(piece) if q & 1 else piece)
    reads_path = tmp_path / "reads.fa"
    reads_path.write_bytes(b"".join(b">read%d cut\n%s\n" % (q, r) for q, r in enumerate(reads)))
    r_list, q_list = (I.as_seed_list(MM.lists(x, k, w, BYTES, NORMALIZE, order)) for x in (recs, reads))
    status, (a_offsets, ref, rev, rpos, qpos, rows), total = M.match(M.Index(r_list), q_list, max_occ)
    want = []
    for q in range(len(reads)):
        lo, hi = int(a_offsets[q]), int(a_offsets[q + 1])
        want.append("read%d\t%d\t%d\t%d\t%d\t%d" % (q, *rows[q].tolist(), hi - lo))
        if "-a" in args:
            want += ["\t%s\t%d\t%d\t%d" % (names[int(ref[i])], rev[i], rpos[i], qpos[i]) for i in range(lo, hi)]
    r = subprocess.run([exe, *args, path, str(reads_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert total > 100 and r.stdout.splitlines() == want
