"""The mapping library (include_pending/needletail_amd/mapping.h, needletail_amd.ChainMappings and ReadMapper) on a real MI355X, exact
against the host model (tests/_mapping_model.py), field by field: rows, order, out_offsets, out, read rows and the stats.  The inputs
are those of tests/_mapping_inputs.py, which tests/test_mapping_inputs.py proves non-vacuous without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import _mapping_inputs as I
import _mapping_model as M
import _stream_order as S
import needletail_amd as nt
from needletail_amd import mapping as MP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = M.W


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "these tests need a GPU"
    c = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev_chains(ch):
    """The chains as device tensors (int64 offsets, int32 words), exactly as long as the arrays: ((c_offsets, chain_rows, m_offsets,
    members), (rpos, qpos))."""
    wide = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()   # noqa: E731
    word = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32).copy()).cuda()   # noqa: E731
    out = (wide(ch.c_offsets), word(ch.chain_rows), wide(ch.m_offsets), word(ch.members)), (word(ch.rpos), word(ch.qpos))
    torch.cuda.synchronize()
    return out


def args_of(p):
    return dict(k=p.k, mask_level=p.mask_level_pm / 1000, pri_ratio=p.pri_ratio_pm / 1000, best_n=p.best_n, min_chain_score=p.min_chain_score)


def assert_result(got, want, what):
    for name, g, w in zip(M.FIELDS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0].tolist()
            raise AssertionError((what, name, at, g[tuple(at)], w[tuple(at)]))


def mapped(mp, ch, p, what=None, dev=None):
    """Mark `ch` (uploaded, or the tensors `dev`) and hold the whole result and the stats to the model."""
    mp.run(*(dev_chains(ch) if dev is None else dev), **args_of(p))
    want = M.run(ch, p)
    assert_result(mp.read(), want, what)
    st = mp.stats()
    assert list(st) == list(M.STATS) and {k: v for k, v in st.items() if k != "device_bytes"} == M.stats(ch, want), what
    return want


def status_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except nt.NtkError as e:
        return e.status
    return M.OK


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------

def test_empty_and_tiny(ctx):
    assert [MP.per_mille(p.mask_level_pm / 1000) for p in I.MASK_PARAMS + (I.DEFAULT,)] == [0, 1000, 1, 999, 500]
    with nt.ChainMappings(ctx) as mp:
        assert mp.read()[0].shape == (0, 16) and mp.device_arrays() == (0,) * 7
        assert mp.stats() == {**M.EMPTY_STATS, "device_bytes": 0}
        for name, ch in I.tiny_cases().items():
            want = mapped(mp, ch, I.DEFAULT, name)
            assert want.out.size == (0 if name in ("no reads", "no chains") else 1)


@pytest.mark.parametrize("name", ["roots", "boundary", "ties", "secondaries", "spans", "mapq"])
def test_fabricated_case(ctx, name):
    """Roots, not links; the mask boundary with mask levels of 0 and 1000; ties; secondaries at the ratio's boundary and best_n of 0, 1,
    5 of 7; both strands and the spans; the mapping quality at its clamps and caps."""
    make, params = I.CASES[name]
    ch = make()
    d = dev_chains(ch)
    with nt.ChainMappings(ctx) as mp:
        for p in params:
            mapped(mp, ch, p, (name, p), d)


def test_strip_seams(ctx):
    """Reads of 1, 2, 63, 64, 65, 128, 129 and 200 chains whose last chain overlaps only the chain of rank 0, 63, 64 or exactly one
    strip back; then reads of 600 and 700 chains, which do not fit the LDS strip buffer."""
    with nt.ChainMappings(ctx) as mp:
        want = mapped(mp, I.seams_case(), I.DEFAULT, "seams")
        assert want.read_rows[1:, 2].tolist() == [1] * (len(I.seam_reads()) - 1)
        want = mapped(mp, I.big_reads_case(), I.DEFAULT, "more chains than the LDS buffer")
        assert want.read_rows[:, 0].min() > MP.LDS_CHAINS and mp.stats()["most_chains"] == 700


def test_more_reads_than_one_step_of_the_capped_grid(ctx):
    """1.25 steps of reads of 1 to 3 chains, worked out from the device's CU count and the rule header's factors."""
    ch, step = I.many_reads_case(n_cu())
    assert step == n_cu() * M.BLOCKS_PER_CU * (M.THREADS // 64)
    with nt.ChainMappings(ctx) as mp:
        mapped(mp, ch, I.DEFAULT, "many reads")
        assert mp.stats()["n_reads"] == step + step // 4 and mp.stats()["most_chains"] == 3


@pytest.mark.parametrize("seed", I.RANDOM_SEEDS)
def test_random_reads(ctx, seed):
    ch = I.random_case(seed)
    d = dev_chains(ch)
    with nt.ChainMappings(ctx) as mp:
        for p in I.RANDOM_PARAMS:
            mapped(mp, ch, p, ("random", seed, p), d)


def test_refusals_leave_the_held_result_unchanged(ctx):
    """One input per flag of the verification, bad parameters and the refusals before any device call: the held result is bit for bit
    what it was.  Then the accepted edges, and reads of 65 535 and 65 536 chains."""
    ch = I.roots_case()
    with nt.ChainMappings(ctx) as mp:
        d = dev_chains(ch)
        before = mapped(mp, ch, I.DEFAULT, "before", d)
        arrays, st = mp.device_arrays(), mp.stats()

        def unchanged(what):
            assert_result(mp.read(), before, what)
            assert mp.device_arrays() == arrays and mp.stats() == st, what

        for what, bad, status in I.refused_cases():
            assert M.verify(bad, I.K) == status
            assert status_of(mp.run, *dev_chains(bad), **args_of(I.DEFAULT)) == status, what
            unchanged(what)
        lib, h = MP.lib(), mp._h
        ptrs = [C.c_void_p(t.data_ptr()) for t in d[0] + d[1]]
        sizes = [ch.c_offsets.size - 1, ch.chain_rows.shape[0], ch.members.size, ch.rpos.size]
        for p in I.bad_params():
            assert M.check_params(p) == M.ERR_BAD_ARG
            params = MP.Params(p.k, p.mask_level_pm, p.pri_ratio_pm, p.best_n, p.min_chain_score, (C.c_uint32 * 3)(p.r0, p.r1, p.r2))
            assert lib.ntk_mapping_run_device(h, *ptrs, *sizes, C.byref(params)) == M.ERR_BAD_ARG, p
            unchanged(p)
        good = MP.Params(I.K, 500, 800, 5, 40)
        call = lambda p, s: lib.ntk_mapping_run_device(h, *p, *s, C.byref(good))   # noqa: E731
        assert call(ptrs, [sizes[0], 1 << 32] + sizes[2:]) == M.ERR_BAD_ARG and call(ptrs, [1 << 32] + sizes[1:]) == M.ERR_BAD_ARG
        for i in range(6):
            assert call(ptrs[:i] + [None] + ptrs[i + 1:], sizes) == M.ERR_BAD_ARG, i
            assert call(ptrs[:i] + [C.c_void_p(ptrs[i].value + 2)] + ptrs[i + 1:], sizes) == M.ERR_BAD_ARG, i
        assert call([C.c_void_p(ptrs[0].value + 4)] + ptrs[1:], sizes) == M.ERR_BAD_ARG
        assert lib.ntk_mapping_run_device(h, *ptrs, *sizes, None) == M.ERR_BAD_ARG
        with pytest.raises(ValueError):
            mp.run(*d, 1 << 32)
        unchanged("the host-side refusals")
        for what, edge in I.accepted_edges().items():
            mapped(mp, edge, I.DEFAULT, what)
        before = mapped(mp, ch, I.DEFAULT, "before, again", d)
        arrays, st = mp.device_arrays(), mp.stats()
        # reads of 2^16 - 1 and 2^16 chains, all on one interval, one member each, scores descending with the index
        for n, status in ((M.READ_CHAINS, M.ERR_UNSUPPORTED), (M.READ_CHAINS - 1, M.OK)):
            rows = torch.zeros((n, 8), dtype=torch.int32, device="cuda")
            rows[:, 0] = 70000 - torch.arange(n, dtype=torch.int32, device="cuda")
            rows[:, 1] = 1
            one = torch.zeros(1, dtype=torch.int32, device="cuda")
            chains = (torch.tensor([0, n], dtype=torch.int64, device="cuda"), rows.reshape(-1), torch.arange(n + 1, dtype=torch.int64, device="cuda"),
                      torch.zeros(n, dtype=torch.int32, device="cuda"))
            torch.cuda.synchronize()
            assert status_of(mp.run, chains, (one, one), **args_of(I.DEFAULT)) == status, n
            if status != M.OK:
                unchanged("a read of 2^16 chains")
        # every chain overlaps the chain of rank 0: one primary, and 5 kept of the eligible (800 per mille of 70 000 is 56 000)
        got_rows, order, out_offsets, out, read_rows = mp.read()
        n = M.READ_CHAINS - 1
        assert read_rows.tolist() == [[n, 1, 5, 0]] and out.tolist() == [0, 1, 2, 3, 4, 5] and out_offsets.tolist() == [0, 6]
        assert np.array_equal(order, np.arange(n, dtype=np.uint32)) and np.array_equal(got_rows[:, F["rank"]], order)
        assert not got_rows[:, F["parent"]].any() and got_rows[0].tolist() == [0, I.K, 0, I.K, 0, 70000, 1, I.K, I.K, 0, 69999, n - 1, 0, 1, 0, 0]
        assert got_rows[1:6, F["flags"]].tolist() == [2] * 5 and not got_rows[6:, F["flags"]].any() and not got_rows[:, F["mapq"]].any()
        assert mp.stats()["most_chains"] == n and mp.stats()["n_reported"] == 6


def test_read_capacities(ctx):
    """The size query and NTK_ERR_CAPACITY of read: one capacity for chains, one for out; nothing is written."""
    ch = I.secondaries_case()
    with nt.ChainMappings(ctx) as mp:
        want = mapped(mp, ch, I.DEFAULT, "capacities")
        lib, h = MP.lib(), mp._h
        n_c, n_o = C.c_uint64(0), C.c_uint64(0)
        assert lib.ntk_mapping_read(h, None, None, None, None, None, 0, 0, C.byref(n_c), C.byref(n_o)) == M.ERR_CAPACITY
        assert (n_c.value, n_o.value) == (17, 11) == (want.rows.shape[0], want.out.size)
        rows, order = np.full((17, 16), 77, dtype=np.uint32), np.full(17, 77, dtype=np.uint32)
        out_offsets, out = np.full(3, 77, dtype=np.uint64), np.full(11, 77, dtype=np.uint32)
        ptr = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        for cap_c, cap_o in ((16, 11), (17, 10)):
            assert lib.ntk_mapping_read(h, ptr(rows), ptr(order), ptr(out_offsets), ptr(out), None, cap_c, cap_o, C.byref(n_c), C.byref(n_o)) == M.ERR_CAPACITY
            assert (n_c.value, n_o.value) == (17, 11) and all((a == 77).all() for a in (rows, order, out_offsets, out))
        assert lib.ntk_mapping_read(h, ptr(rows), ptr(order), ptr(out_offsets), ptr(out), None, 17, 11, C.byref(n_c), C.byref(n_o)) == M.OK
        assert np.array_equal(rows, want.rows) and np.array_equal(order, want.order) and np.array_equal(out, want.out)
        assert np.array_equal(out_offsets, want.out_offsets)
        assert lib.ntk_mapping_read(h, None, None, None, None, None, 17, 11, C.byref(n_c), C.byref(n_o)) == M.ERR_BAD_ARG


class _DeviceView:
    def __init__(self, address, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (address, False), "version": 2}


def test_held_memory(ctx):
    """stats.device_bytes is the model's, exactly: after a run, after a smaller run (the arrays stay), after trim (nothing is held) and
    after the run that follows; result_device is what read returns; a second run replaces the first."""
    large, small = I.random_case(I.RANDOM_SEEDS[0]), I.secondaries_case()
    with nt.ChainMappings(ctx) as mp:
        want = mapped(mp, large, I.DEFAULT, "large")
        sizes = lambda c, w: dict(n_reads=c.c_offsets.size - 1, n_chains=c.chain_rows.shape[0], n_reported=w.out.size)   # noqa: E731
        big = sizes(large, want)
        assert mp.stats()["device_bytes"] == M.device_bytes(**big), "rocPRIM's temporary storage is not held"
        first = mapped(mp, small, I.DEFAULT, "smaller")
        assert mp.stats()["device_bytes"] == M.device_bytes(**big), "every array keeps the largest size needed so far"
        arrays = mp.device_arrays()
        d_rows, d_order, d_out_offsets, d_out, d_read_rows, n_c, n_o = arrays
        assert (n_c, n_o) == (17, 11) and all(arrays[:5])
        clone = lambda a, m, t: torch.as_tensor(_DeviceView(a, m, t), device="cuda").clone().cpu().numpy()   # noqa: E731
        assert np.array_equal(clone(d_rows, 17 * 16, "<i4").view(np.uint32), first.rows.reshape(-1))
        assert np.array_equal(clone(d_order, 17, "<i4").view(np.uint32), first.order)
        assert np.array_equal(clone(d_out_offsets, 3, "<i8").view(np.uint64), first.out_offsets)
        assert np.array_equal(clone(d_out, 11, "<i4").view(np.uint32), first.out)
        assert np.array_equal(clone(d_read_rows, 8, "<i4").view(np.uint32), first.read_rows.reshape(-1))
        assert mp.device_arrays() == arrays
        mp.trim()
        assert mp.stats() == {**M.EMPTY_STATS, "device_bytes": 0} and mp.device_arrays() == (0,) * 7 and mp.read()[0].shape == (0, 16)
        want = mapped(mp, small, I.DEFAULT, "after trim")
        assert mp.stats()["device_bytes"] == M.device_bytes(**sizes(small, want))
        mapped(mp, M.batch_of([]), I.DEFAULT, "an empty batch keeps the arrays")
        assert mp.stats()["device_bytes"] == M.device_bytes(**sizes(small, want))
    with nt.ChainMappings(ctx) as mp:
        mapped(mp, M.batch_of([]), I.DEFAULT, "an empty batch alone")
        assert mp.stats()["device_bytes"] == M.device_bytes(0)


# ---- the stream contract ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available(), "these tests need a GPU"
    S.cycles_per_ms()
    r = S.Rig()
    yield r
    r.close()


def test_stream_order(rig):
    """Every call with work pending on the context's stream: the chains and anchors are produced behind the hold (a decoy of the same
    shape in front) and clobbered behind the call; read, stats and device_arrays are made with that work pending.  run_device, read,
    stats and trim are SYNC; result_device queues nothing and waits for nothing."""
    ch = I.secondaries_case()
    rows = ch.chain_rows.copy()
    rows[:, 0] = rows[::-1, 0]
    decoy = ch._replace(chain_rows=rows, qpos=ch.qpos + np.uint32(7))
    want = M.run(ch, I.DEFAULT)
    assert M.verify(decoy, I.K) == M.OK and not np.array_equal(M.run(decoy, I.DEFAULT).rows, want.rows), "the decoy maps otherwise"
    (tc, ta), (dc, da) = dev_chains(ch), dev_chains(decoy)
    inputs = [S.Input(a, b, 0) for a, b in zip(tc + ta, dc + da)]
    with nt.ChainMappings(rig.ctx) as mp:
        def run():
            bufs = tuple(i.buf for i in inputs)
            mp.run(bufs[:4], bufs[4:], **args_of(I.DEFAULT))

        def read():
            arrays = mp.device_arrays()
            return mp.read(), mp.stats(), arrays

        for plain in (True, False):
            _, _, (got, st, arrays) = S.hazard_call(rig, S.SYNC, inputs, [], run, read, plain=plain)
            assert_result(got, want, ("stream order", plain))
            assert st["n_chains"] == 17 == arrays[5] and st["n_reported"] == 11 == arrays[6]
        S.hazard_call(rig, S.SYNC, [], [], mp.read)
        S.hazard_call(rig, S.SYNC, [], [], mp.stats)
        S.hazard_call(rig, S.ASYNC, [], [], mp.device_arrays)   # with the hold pending: it returns before the stream drains
        S.hazard_call(rig, S.SYNC, [], [], mp.trim)             # with a hold pending it has to wait for the stream first
        assert mp.stats()["n_reads"] == 0 and mp.read()[0].shape == (0, 16)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------

def test_end_to_end_read_mapper(ctx):
    """ReadMapper on three random references, the third with one segment planted twice.  Reads cut forward and reverse-complemented
    from unique sequence map to where they were cut, with mapq 60, and are primary; reads cut from the segment report one primary with
    mapq 0 and one kept secondary at the other copy.  The rows are the model's on the chains and anchors read back."""
    k = 15
    refs, reads, cuts = I.sequences()
    assert len(reads) <= 200
    read_len = len(reads[0])
    with nt.ReadMapper(k, 10, ctx=ctx) as rm:
        rm.index_records(refs)
        got = rm.map_records(reads)
        c_offsets, chain_rows, m_offsets, members, _, _, _ = rm.chains.read()
        _, _, _, rpos, qpos, _ = rm.seeds.read()
        held = rm.mappings.read()
    ch = M.Chains(c_offsets, chain_rows, m_offsets, members, rpos, qpos)
    want = M.run(ch, M.Params(k))
    assert_result(held, want, "end to end")
    sel = want.rows[want.out]
    assert got.dtype == MP.MAPPING and got.size == want.out.size
    assert np.array_equal(got["read"], np.repeat(np.arange(len(reads)), np.diff(want.out_offsets.astype(np.int64))))
    for name in ("qs", "qe", "rs", "re", "mlen", "blen", "mapq", "score", "cnt"):
        assert np.array_equal(got[name], sel[:, F[name]]), name
    assert np.array_equal(got["ref"], sel[:, F["ref_rev"]] >> 1) and np.array_equal(got["strand"] == b"-", sel[:, F["ref_rev"]] & 1 == 1)
    assert np.array_equal(got["primary"], sel[:, F["flags"]] & 1 == 1)
    for q, cut in enumerate(cuts):
        mine = got[got["read"] == q]
        if len(cut) == 3:
            (r, rev, start), m = cut, mine[0]
            assert len(mine) == 1 and m["primary"] and m["mapq"] == 60 and m["ref"] == r and m["strand"] == (b"-" if rev else b"+"), q
            assert start <= m["rs"] < m["re"] <= start + read_len and 0 <= m["qs"] < m["qe"] <= read_len and m["re"] - m["rs"] > read_len // 2, q
            assert m["rs"] - start == (read_len - m["qe"] if rev else m["qs"]), q
        else:
            r, rev, start, other = cut
            assert len(mine) == 2 and mine["primary"].tolist() == [True, False] and mine["mapq"].tolist() == [0, 0], q
            assert set(mine["ref"].tolist()) == {r} and set(mine["strand"].tolist()) == {b"-" if rev else b"+"}, q
            starts = sorted(int(m["rs"] - (read_len - m["qe"] if rev else m["qs"])) for m in mine)
            assert starts == [start, other], q


# ---- the example program ------------------------------------------------------------------------------------------------------------------

def test_example_program_writes_paf(tmp_path):
    """examples/map_reads on the sequences of the end-to-end test: twelve PAF columns and the tags, the rows ReadMapper gives."""
    exe = os.path.join(ROOT, "examples", "map_reads")
    refs, reads, cuts = I.sequences()
    ref_path, read_path = tmp_path / "refs.fa", tmp_path / "reads.fa"
    ref_path.write_bytes(b"".join(b">ref%d some words\n%s\n" % (i, r) for i, r in enumerate(refs)))
    read_path.write_bytes(b"".join(b">read%d cut\n%s\n" % (q, r) for q, r in enumerate(reads)))
    with nt.ReadMapper(15, 10) as rm:
        rm.index_records(refs)
        got = rm.map_records(reads)
        rows, _, _, out, _ = rm.mappings.read()
    want = []
    for m, c in zip(got, out.tolist()):
        want.append("read%d\t%d\t%d\t%d\t%s\tref%d\t%d\t%d\t%d\t%d\t%d\t%d\ttp:A:%s\ts1:i:%d\ts2:i:%d\tcm:i:%d" % (
            m["read"], len(reads[m["read"]]), m["qs"], m["qe"], m["strand"].decode(), m["ref"], len(refs[m["ref"]]), m["rs"], m["re"], m["mlen"],
            m["blen"], m["mapq"], "P" if m["primary"] else "S", m["score"], rows[c, F["subsc"]], m["cnt"]))
    r = subprocess.run([exe, str(ref_path), str(read_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert len(want) >= len(reads) and r.stdout.splitlines() == want
