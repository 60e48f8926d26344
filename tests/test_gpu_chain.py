"""The chain library (include_pending/needletail_amd/chain.h, needletail_amd.AnchorChains) on a real MI355X, exact against the host
model (tests/_chain_model.py), field by field: c_offsets, chain rows, m_offsets, members, f, p, read rows and the stats.  The inputs are
those of tests/_chain_inputs.py, which tests/test_chain_inputs.py proves non-vacuous without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import _chain_inputs as I
import _chain_model as M
import _minimizer_list_model as MM
import _seed_index_inputs as SI
import _seed_index_model as SM
import _stream_order as S
import needletail_amd as nt
from needletail_amd import chaining as CH

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    assert torch.cuda.is_available(), "these tests need a GPU"
    c = nt.Context(0, stream=torch.cuda.current_stream().cuda_stream)
    yield c
    c.close()


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev_anchors(anchors):
    """The anchors as four device tensors (int64 offsets, int32 triples), exactly as long as the arrays."""
    off, ref_rev, rpos, qpos = anchors
    out = (torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64).copy()).cuda(),) + tuple(
        torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).cuda() for a in (ref_rev, rpos, qpos))
    torch.cuda.synchronize()
    return out


def args_of(p):
    return dict(k=p.k, max_dist=p.max_dist, bw=p.bw, h=p.h, min_score=p.min_score, min_cnt=p.min_cnt)


def assert_result(got, want, what):
    for name, g, w in zip(M.FIELDS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), (what, name)


def chained(ch, anchors, p, what=None, dev=None):
    """Chain `anchors` (uploaded, or the tensors `dev`) and hold the whole result and the stats to the model."""
    ch.run(dev_anchors(anchors) if dev is None else dev, **args_of(p))
    want = M.chain(anchors, p)
    got = ch.read()
    assert_result(got, want, what)
    st = ch.stats()
    assert list(st) == list(M.STATS) and {k: v for k, v in st.items() if k != "device_bytes"} == M.stats(anchors, p, want), what
    return want


def status_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except nt.NtkError as e:
        return e.status
    return M.OK


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------

def test_empty_and_tiny(ctx):
    with nt.AnchorChains(ctx) as ch:
        assert ch.read()[1].shape == (0, 8) and ch.device_arrays() == (0,) * 9
        assert {k: v for k, v in ch.stats().items()} == {**M.EMPTY_STATS, "device_bytes": 0}
        for name, anchors in I.tiny_cases().items():
            want = chained(ch, anchors, I.DEFAULT, name)
            assert want.chain_rows.shape[0] == (1 if name == "anchors among empty reads" else 0)
        chained(ch, I.tiny_cases()["two anchors"], M.Params(I.K, min_score=20, min_cnt=2), "two anchors, kept")
    for (anchors, f) in I.fixtures():
        with nt.AnchorChains(ctx) as ch:
            assert chained(ch, anchors, I.DEFAULT, "fixture").f.tolist() == f


def test_strands_and_references(ctx):
    with nt.AnchorChains(ctx) as ch:
        want = chained(ch, I.strands_case(), I.DEFAULT, "strands")
        assert want.chain_rows[:, 2].tolist() == [1, 0, 2, 5]


@pytest.mark.parametrize("h", I.WINDOW_H)
def test_the_window_at_the_strip_seams(ctx, h):
    """A run whose last anchor's only good predecessor lies exactly h back (inside the window) and h + 1 back (outside)."""
    p = M.Params(I.K, h=h)
    with nt.AnchorChains(ctx) as ch:
        assert chained(ch, I.window_case(h), p, ("window", h)).f[-1] == 30
        assert chained(ch, I.window_case(h + 1), p, ("window + 1", h)).f[-1] == 15


def test_ties(ctx):
    with nt.AnchorChains(ctx) as ch:
        want = chained(ch, I.ties_case(), I.DEFAULT, "ties")
        assert want.p[2] == 1 and want.chain_rows[:, :3].tolist() == [[60, 4, 0], [60, 4, 2]]


def test_edges_of_the_pair_rule(ctx):
    with nt.AnchorChains(ctx) as ch:
        want = chained(ch, I.pair_edges_case(), I.EDGE_PARAMS, "pair edges")
        assert [bool(want.p[2 * q + 1] != M.NONE) for q in range(len(I.pair_edge_reads()))] == [follows for _, follows in I.pair_edge_reads().values()]
        for k, (anchors, p) in I.k_cases().items():
            chained(ch, anchors, p, ("k", k))
        chained(ch, I.k_cases()[255][0], M.Params(255, max_dist=(1 << 31) - 1, bw=(1 << 31) - 1, h=512, min_score=(1 << 32) - 1, min_cnt=(1 << 32) - 1), "the largest parameters")


def test_run_seams(ctx):
    with nt.AnchorChains(ctx) as ch:
        chained(ch, I.run_seams_case(), I.SEAM_PARAMS, "run seams")
        assert ch.stats()["n_runs"] == 9 and ch.stats()["longest_run"] == 2


def test_forks(ctx):
    with nt.AnchorChains(ctx) as ch:
        want = chained(ch, I.forks_case(), I.DEFAULT, "forks")
        assert want.read_rows.tolist() == [[15, 2, 15, 150], [13, 1, 10, 150]] and want.chain_rows[1, :2].tolist() == [57, 5]
        assert chained(ch, I.forks_case(), I.MIN_CNT_PARAMS, "forks, min_cnt").read_rows[0].tolist() == [15, 1, 10, 150]
        want = chained(ch, I.marked_case(), I.MARKED_PARAMS, "a chain stops at an anchor a dropped chain marked")
        assert want.chain_rows[0, :2].tolist() == [53, 20]


def test_one_run_of_5000_anchors(ctx):
    with nt.AnchorChains(ctx) as ch:
        anchors = I.long_run_case()
        d = dev_anchors(anchors)
        chained(ch, anchors, I.DEFAULT, "one long run", d)
        assert ch.stats()["longest_run"] == anchors[1].size > 4900 and ch.stats()["n_runs"] == 1
        chained(ch, anchors, M.Params(I.K, h=130, max_dist=100, bw=30), "one long run, three strips and the early way out", d)


def test_more_runs_than_one_step_of_the_capped_grid(ctx):
    """1.25 steps of one-anchor runs and as many three-anchor runs, worked out from the device's CU count and the rule header's factors."""
    anchors, step = I.many_runs_case(n_cu())
    assert step == n_cu() * M.BLOCKS_PER_CU * (M.THREADS // 64)
    with nt.AnchorChains(ctx) as ch:
        chained(ch, anchors, I.DEFAULT, "many runs")
        assert ch.stats()["n_runs"] > 5 * step // 2 and ch.stats()["longest_run"] == 3


@pytest.mark.parametrize("seed", I.RANDOM_SEEDS)
def test_random_reads_with_planted_chains(ctx, seed):
    anchors = I.random_case(seed)
    d = dev_anchors(anchors)
    with nt.AnchorChains(ctx) as ch:
        for p in I.RANDOM_PARAMS:
            chained(ch, anchors, p, ("random", seed, p), d)


def test_end_to_end_from_sequences(ctx):
    """Reads sampled from random references on both strands with 1 % substitutions go through MinimizerList, SeedIndex and AnchorChains
    on the device; the result is the model's on the anchors read back, and every read's best chain lies on its origin reference, strand
    and diagonal."""
    k, w = 15, 10
    refs, reads, cuts = I.sequences()
    with nt.MinimizerList(k, nt.PATH_BITS_CANONICAL, w, nt.HASH, ctx) as r_ml, nt.MinimizerList(k, nt.PATH_BITS_CANONICAL, w, nt.HASH, ctx) as q_ml, \
            nt.SeedIndex(ctx) as si, nt.AnchorChains(ctx) as ch:
        r_ml.run_records(refs, nt.PRE_NORMALIZE)
        q_ml.run_records(reads, nt.PRE_NORMALIZE)
        si.build(r_ml)
        si.match(q_ml)
        ch.run(si, k)
        a_offsets, ref, rev, rpos, qpos, _ = si.read()
        got, st = ch.read(), ch.stats()
    anchors = M.as_anchors(a_offsets, ref.astype(np.uint32) << 1 | rev, rpos, qpos)
    want = M.chain(anchors, I.DEFAULT)
    assert_result(got, want, "end to end")
    assert {k_: v for k_, v in st.items() if k_ != "device_bytes"} == M.stats(anchors, I.DEFAULT, want)
    read_len = len(reads[0])
    for q, (r, is_rev, start) in enumerate(cuts):
        lo, hi = int(want.c_offsets[q]), int(want.c_offsets[q + 1])
        assert hi > lo, q
        best = max(range(lo, hi), key=lambda c: (int(want.chain_rows[c, 0]), -c))
        score, n, ref_rev, r0, q0, r1, q1, _ = want.chain_rows[best].tolist()
        assert score == want.read_rows[q, 3] and ref_rev == r << 1 | is_rev and n >= 10, q
        # a k-mer at qpos of the read lies at start + qpos of the reference, or - reverse - at start + read_len - k - qpos
        for rp, qp in ((r0, q0), (r1, q1)):
            assert rp == (start + read_len - k - qp if is_rev else start + qp), q


def test_refusals_leave_the_held_result_unchanged(ctx):
    """Unsorted anchors, a repeated anchor, decreasing offsets, offsets[n_reads] > n, bad parameters and a non-zero reserved word: the
    held result is bit for bit what it was.  Then the refusals that come before any device call, and a read of 2^23 anchors."""
    anchors = I.strands_case()
    with nt.AnchorChains(ctx) as ch:
        d = dev_anchors(anchors)
        before = chained(ch, anchors, I.DEFAULT, "before", d)
        arrays, st = ch.device_arrays(), ch.stats()

        def unchanged(what):
            assert_result(ch.read(), before, what)
            assert ch.device_arrays() == arrays and ch.stats() == st, what

        for what, bad, status in I.refused_cases():
            assert M.verify(bad) == status
            assert status_of(ch.run, dev_anchors(bad), **args_of(I.DEFAULT)) == status, what
            unchanged(what)
        lib, h = CH.lib(), ch._h
        ptrs = [C.c_void_p(t.data_ptr()) for t in d]
        n_reads, n = anchors[0].size - 1, anchors[1].size
        for p in I.bad_params():
            assert M.check_params(p) == M.ERR_BAD_ARG
            params = CH.Params(p.k, p.max_dist, p.bw, p.h, p.min_score, p.min_cnt, (C.c_uint32 * 2)(p.r0, p.r1))
            assert lib.ntk_chain_run_device(h, *ptrs, n_reads, n, C.byref(params)) == M.ERR_BAD_ARG, p
            unchanged(p)
        good = CH.Params(*I.DEFAULT[:6])
        call = lambda *a: lib.ntk_chain_run_device(h, *a, C.byref(good))   # noqa: E731
        assert call(*ptrs, n_reads, 1 << 32) == M.ERR_BAD_ARG and call(*ptrs, 1 << 31, n) == M.ERR_BAD_ARG
        assert call(None, *ptrs[1:], n_reads, n) == M.ERR_BAD_ARG and call(ptrs[0], None, *ptrs[2:], n_reads, n) == M.ERR_BAD_ARG
        assert call(C.c_void_p(ptrs[0].value + 4), *ptrs[1:], n_reads, n) == M.ERR_BAD_ARG
        assert call(*ptrs[:3], C.c_void_p(ptrs[3].value + 2), n_reads, n) == M.ERR_BAD_ARG
        assert lib.ntk_chain_run_device(h, *ptrs, n_reads, n, None) == M.ERR_BAD_ARG
        unchanged("the host-side refusals")
        # a read of 2^23 anchors, sorted: NTK_ERR_UNSUPPORTED
        m = M.READ_ANCHORS
        ramp = torch.arange(m, dtype=torch.int32, device="cuda")
        long_read = (torch.tensor([0, m], dtype=torch.int64, device="cuda"), torch.zeros(m, dtype=torch.int32, device="cuda"), ramp, ramp)
        torch.cuda.synchronize()
        assert status_of(ch.run, long_read, **args_of(I.DEFAULT)) == M.ERR_UNSUPPORTED
        unchanged("a read of 2^23 anchors")
        chained(ch, anchors, I.DEFAULT, "after", d)


def test_read_capacities(ctx):
    """The size query and NTK_ERR_CAPACITY of read: one capacity for chains, one for members; nothing is written."""
    anchors = I.strands_case()
    with nt.AnchorChains(ctx) as ch:
        want = chained(ch, anchors, I.DEFAULT, "capacities")
        lib, h = CH.lib(), ch._h
        n_c, n_m = C.c_uint64(0), C.c_uint64(0)
        assert lib.ntk_chain_read(h, None, None, None, None, None, None, None, 0, 0, C.byref(n_c), C.byref(n_m)) == M.ERR_CAPACITY
        assert (n_c.value, n_m.value) == (4, 22) == (want.chain_rows.shape[0], want.members.size)
        c_offsets, rows = np.full(3, 77, dtype=np.uint64), np.full((4, 8), 77, dtype=np.uint32)
        m_offsets, members = np.full(5, 77, dtype=np.uint64), np.full(22, 77, dtype=np.uint32)
        ptr = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        for cap_c, cap_m in ((3, 22), (4, 21)):
            assert lib.ntk_chain_read(h, ptr(c_offsets), ptr(rows), ptr(m_offsets), ptr(members), None, None, None, cap_c, cap_m,
                                      C.byref(n_c), C.byref(n_m)) == M.ERR_CAPACITY
            assert (n_c.value, n_m.value) == (4, 22) and all((a == 77).all() for a in (c_offsets, rows, m_offsets, members))
        assert lib.ntk_chain_read(h, ptr(c_offsets), ptr(rows), ptr(m_offsets), ptr(members), None, None, None, 4, 22, C.byref(n_c), C.byref(n_m)) == M.OK
        assert np.array_equal(c_offsets, want.c_offsets) and np.array_equal(rows, want.chain_rows) and np.array_equal(members, want.members)
        assert lib.ntk_chain_read(h, None, None, None, None, None, None, None, 4, 22, C.byref(n_c), C.byref(n_m)) == M.ERR_BAD_ARG


class _DeviceView:
    def __init__(self, address, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (address, False), "version": 2}


def test_held_memory(ctx):
    """stats.device_bytes is the model's, exactly: after a run, after a smaller run (the arrays stay), after trim (nothing is held) and
    after the run that follows; result_device is what read returns; a second run replaces the first."""
    large, small = I.random_case(I.RANDOM_SEEDS[0]), I.strands_case()
    with nt.AnchorChains(ctx) as ch:
        want = chained(ch, large, I.DEFAULT, "large")
        sizes = lambda a, w, s: dict(n_reads=a[0].size - 1, n_anchors=a[1].size, n_runs=s["n_runs"], n_chains=w.chain_rows.shape[0], n_members=w.members.size)   # noqa: E731
        big = sizes(large, want, ch.stats())
        assert ch.stats()["device_bytes"] == M.device_bytes(**big), "rocPRIM's temporary storage is not held"
        first = chained(ch, small, I.DEFAULT, "smaller")
        assert ch.stats()["device_bytes"] == M.device_bytes(**big), "every array keeps the largest size needed so far"
        arrays = ch.device_arrays()
        d_c_offsets, d_chain_rows, d_m_offsets, d_members, d_f, d_p, d_read_rows, n_c, n_m = arrays
        assert (n_c, n_m) == (4, 22) and all(arrays[:7])
        clone = lambda a, m, t: torch.as_tensor(_DeviceView(a, m, t), device="cuda").clone().cpu().numpy()   # noqa: E731
        assert np.array_equal(clone(d_c_offsets, 3, "<i8").view(np.uint64), first.c_offsets)
        assert np.array_equal(clone(d_chain_rows, 32, "<i4").view(np.uint32), first.chain_rows.reshape(-1))
        assert np.array_equal(clone(d_m_offsets, 5, "<i8").view(np.uint64), first.m_offsets)
        assert np.array_equal(clone(d_members, 22, "<i4").view(np.uint32), first.members)
        assert np.array_equal(clone(d_f, 22, "<i4"), first.f) and np.array_equal(clone(d_p, 22, "<i4").view(np.uint32), first.p)
        assert np.array_equal(clone(d_read_rows, 8, "<i4").view(np.uint32), first.read_rows.reshape(-1))
        assert ch.device_arrays() == arrays
        ch.trim()
        assert ch.stats() == {**M.EMPTY_STATS, "device_bytes": 0} and ch.device_arrays() == (0,) * 9 and ch.read()[1].shape == (0, 8)
        want = chained(ch, small, I.DEFAULT, "after trim")
        assert ch.stats()["device_bytes"] == M.device_bytes(**sizes(small, want, ch.stats()))
        empty = M.reads_of([])
        chained(ch, empty, I.DEFAULT, "an empty batch keeps the arrays")
        assert ch.stats()["device_bytes"] == M.device_bytes(**sizes(small, want, {"n_runs": 4}))
    with nt.AnchorChains(ctx) as ch:
        chained(ch, M.reads_of([]), I.DEFAULT, "an empty batch alone")
        assert ch.stats()["device_bytes"] == M.device_bytes(0)
        with pytest.raises(ValueError):
            ch.run(dev_anchors(small), 1 << 32)


# ---- the stream contract ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available(), "these tests need a GPU"
    S.cycles_per_ms()
    r = S.Rig()
    yield r
    r.close()


def test_stream_order(rig):
    """Every call with work pending on the context's stream: the anchors are produced behind the hold (a decoy of the same shape in
    front) and clobbered behind the call; read, stats and device_arrays are made with that work pending.  run_device, read, stats and
    trim are SYNC; result_device queues nothing and waits for nothing."""
    anchors = I.strands_case()
    decoy = (anchors[0], anchors[1], anchors[2] + np.uint32(1000), anchors[3])
    want = M.chain(anchors, I.DEFAULT)
    assert M.verify(decoy) == M.OK and not np.array_equal(M.chain(decoy, I.DEFAULT).chain_rows, want.chain_rows), "the decoy chains otherwise"
    inputs = [S.Input(a, b, 0) for a, b in zip(dev_anchors(anchors), dev_anchors(decoy))]
    with nt.AnchorChains(rig.ctx) as ch:
        def run():
            ch.run(tuple(i.buf for i in inputs), **args_of(I.DEFAULT))

        def read():
            arrays = ch.device_arrays()
            return ch.read(), ch.stats(), arrays

        for plain in (True, False):
            _, _, (got, st, arrays) = S.hazard_call(rig, S.SYNC, inputs, [], run, read, plain=plain)
            assert_result(got, want, ("stream order", plain))
            assert st["n_chains"] == 4 == arrays[7] and st["n_members"] == 22 == arrays[8]
        S.hazard_call(rig, S.SYNC, [], [], ch.read)
        S.hazard_call(rig, S.SYNC, [], [], ch.stats)
        S.hazard_call(rig, S.ASYNC, [], [], ch.device_arrays)   # with the hold pending: it returns before the stream drains
        S.hazard_call(rig, S.SYNC, [], [], ch.trim)             # with a hold pending it has to wait for the stream first
        assert ch.stats()["n_reads"] == 0 and ch.read()[1].shape == (0, 8)


# ---- the example program ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("args,p", [((), I.DEFAULT), (("-h", "3", "-m", "30", "-n", "2", "-g", "400", "-r", "50"), M.Params(I.K, 400, 50, 3, 30, 2))])
def test_example_program_on_the_golden_28s(tmp_path, args, p):
    """examples/chain_reads on reads of 300 bp cut from the golden 28S sequences, forward and reverse: its lines are the model's chains
    of the model's anchors of the model's lists."""
    exe, path = os.path.join(ROOT, "examples", "chain_reads"), os.path.join(ROOT, "tests", "golden", "28S.fasta")
    k, w = 15, 10
    names, recs = [], []
    for line in open(path, "rb").read().splitlines():
        if line.startswith(b">"):
            names.append(line[1:].split()[0].decode() if line[1:].split() else "")
            recs.append(b"")
        elif recs:
            recs[-1] += line.strip()
    rng = np.random.default_rng(0x286)
    reads = []
    for q in range(30):
        r = int(rng.integers(0, len(recs)))
        s = int(rng.integers(0, max(1, len(recs[r]) - 300)))
        piece = recs[r][s: s + 300].upper()
        reads.append(SI.revcomp(piece) if q & 1 else piece)
    reads_path = tmp_path / "reads.fa"
    reads_path.write_bytes(b"".join(b">read%d cut\n%s\n" % (q, r) for q, r in enumerate(reads)))
    r_list, q_list = (SI.as_seed_list(MM.lists(x, k, w, nt.PATH_BYTES_CANONICAL, nt.PRE_NORMALIZE, MM.HASH)) for x in (recs, reads))
    status, (a_offsets, ref, rev, rpos, qpos, rows), total = SM.match(SM.Index(r_list), q_list, 0)
    got = M.chain(M.as_anchors(a_offsets, ref.astype(np.uint32) << 1 | rev, rpos, qpos), p)
    want = []
    for q in range(len(reads)):
        for c in range(int(got.c_offsets[q]), int(got.c_offsets[q + 1])):
            score, n, ref_rev, r0, q0, r1, q1, _ = got.chain_rows[c].tolist()
            q_start, q_end = (q1, q0 + k) if ref_rev & 1 else (q0, q1 + k)
            want.append("read%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d" % (q, q_start, q_end, "-" if ref_rev & 1 else "+", names[ref_rev >> 1], r0, r1 + k, n, score))
    r = subprocess.run([exe, *args, path, str(reads_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert len(want) >= 30 and r.stdout.splitlines() == want
