"""The alignment library (include_pending/needletail_amd/align.h, needletail_amd.ChainAlignments and ReadMapper.map_aligned) on a real
MI355X, exact against the host model (tests/_align_model.py), field by field: rows, scores, g_offsets, cigar and the stats.  The inputs
are those of tests/_align_inputs.py, which tests/test_align_inputs.py proves non-vacuous without a GPU."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest
import torch

import _align_inputs as I
import _align_model as M
import _stream_order as S
import needletail_amd as nt
from needletail_amd import aligning as AL

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


def _wide(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def _word(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32).copy()).cuda()


def dev_input(inp):
    """The input as device tensors, exactly as long as the arrays: [ref bytes, ref offsets, read bytes, read offsets, c_offsets,
    chain_rows, m_offsets, members, rpos, qpos, sel]."""
    ch = inp.chains
    out = [torch.from_numpy(inp.refs.data.copy()).cuda(), _wide(inp.refs.offsets), torch.from_numpy(inp.reads.data.copy()).cuda(), _wide(inp.reads.offsets),
           _wide(ch.c_offsets), _word(ch.chain_rows), _wide(ch.m_offsets), _word(ch.members), _word(ch.rpos), _word(ch.qpos), _word(inp.sel)]
    torch.cuda.synchronize()
    return out


def run_args(d):
    """The positional arguments of ChainAlignments.run of the tensors of dev_input."""
    return (d[0], d[0].numel(), d[1], d[1].numel() - 1), (d[2], d[2].numel(), d[3], d[3].numel() - 1), tuple(d[4:8]), tuple(d[8:10]), d[10]


def kw_of(p):
    return p._asdict()


def assert_result(got, want, what):
    for name, g, w in zip(M.FIELDS, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        if not np.array_equal(g, w):
            at = np.argwhere(g != w)[0].tolist()
            raise AssertionError((what, name, at, g[tuple(at)], w[tuple(at)]))


_MODEL = {}


def model(name, inp, p):
    """The model's answer for a named input, computed once."""
    key = (name, p._replace(work_mib=0))
    if key not in _MODEL:
        _MODEL[key] = M.run(inp, p)
    return _MODEL[key]


def aligned(al, name, inp, p, dev=None):
    """Align `inp` (uploaded, or the tensors `dev`) and hold the whole result and the stats to the model."""
    al.run(*run_args(dev_input(inp) if dev is None else dev), **kw_of(p))
    want, chains = model(name, inp, p)
    assert_result(al.read(), want, name)
    st = al.stats()
    assert list(st) == list(M.STATS) and {k: v for k, v in st.items() if k != "device_bytes"} == M.stats(inp, p, want, chains), (name, st)
    return want, chains


def status_of(fn, *args, **kw):
    try:
        fn(*args, **kw)
    except nt.NtkError as e:
        return e.status
    return M.OK


def cigars(want):
    return [M.cigar_string(want.cigar[int(a): int(b)]) for a, b in zip(want.g_offsets, want.g_offsets[1:])]


# ---- the cases ----------------------------------------------------------------------------------------------------------------------------

def test_empty_and_tiny(ctx):
    with nt.ChainAlignments(ctx) as al:
        assert al.read()[0].shape == (0, 8) and al.device_arrays() == (0,) * 6
        assert al.stats() == {**M.EMPTY_STATS, "device_bytes": 0}
        for name, (inp, p) in I.tiny_cases().items():
            want, _ = aligned(al, name, inp, p)
            assert want.rows.shape[0] == inp.sel.size
        assert nt.cigar_string(al.read()[3][:5]) == "3=2I3=2D7="


def test_strip_seams(ctx):
    """n = m at 63, 64, 65, 127, 128, 129 and n != m across 64: the strips of 64 rows and the blocks of 64 query codes, on both strands."""
    with nt.ChainAlignments(ctx) as al:
        aligned(al, "seams", I.seams_case(), I.DEFAULT)
        aligned(al, "seams, no padding", I.seams_case(), I.DEFAULT._replace(band_pad=0))
        aligned(al, "seams, band of 3", I.seams_case(), I.DEFAULT._replace(band_pad=1))


@pytest.mark.parametrize("name", list(I.band_cases()))
def test_band(ctx, name):
    inp, p, _ = I.band_cases()[name]
    with nt.ChainAlignments(ctx) as al:
        aligned(al, name, inp, p)


def test_ties_and_bases(ctx):
    """Homopolymers and an adjacent deletion and insertion run; N, break bytes, lower case and U; the scores at their edges."""
    inp, p = I.ties_case()
    with nt.ChainAlignments(ctx) as al:
        want, _ = aligned(al, "ties", inp, p)
        assert cigars(want)[:2] == ["7=1D10=", "7=1I10="] and cigars(want)[6] == "11=4I4D11="
        aligned(al, "bases", I.bases_case(), I.DEFAULT)
        for i, p in enumerate(I.edge_params()):
            aligned(al, "ties, edge params %d" % i, inp, p)
            aligned(al, "seams, edge params %d" % i, I.seams_case(), p)


def test_strands_at_the_ends_of_their_records(ctx):
    at_ends, inside = I.strands_case()
    with nt.ChainAlignments(ctx) as al:
        a, _ = aligned(al, "strands at the ends", at_ends, I.DEFAULT)
        b, _ = aligned(al, "strands inside", inside, I.DEFAULT)
        assert_result(a, b, "the records around a chain do not matter")


def test_max_seg(ctx):
    inp, p, too_long = I.max_seg_case()
    with nt.ChainAlignments(ctx) as al:
        want, _ = aligned(al, "max_seg", inp, p)
        assert np.flatnonzero(want.rows[:, 0] == M.TOO_LONG).tolist() == too_long and al.stats()["n_too_long"] == len(too_long)


def test_largest_segment(ctx):
    """One part of 4095 x 4095 with band_pad = 4095 between two small ones, run once."""
    inp, p = I.largest_case()
    with nt.ChainAlignments(ctx) as al:
        aligned(al, "largest", inp, p)
        assert al.stats()["n_groups"] == 1 and al.stats()["dp_cells"] == 2 * 100 * 100 + I.LARGEST * I.LARGEST


def test_groups(ctx):
    """Three parts of 2400 x 2400: with work_mib = 16 two groups, by default one, with equal results."""
    inp, p = I.groups_case()
    d = dev_input(inp)
    with nt.ChainAlignments(ctx) as al:
        aligned(al, "groups", inp, p._replace(work_mib=16), d)
        assert al.stats()["n_groups"] == 2
        first = al.read()
        aligned(al, "groups", inp, p, d)
        assert al.stats()["n_groups"] == 1
        assert_result(al.read(), first, "groups")


def test_selection_with_duplicates_in_any_order(ctx):
    with nt.ChainAlignments(ctx) as al:
        want, _ = aligned(al, "selection", I.selection_case(), I.DEFAULT)
        c = cigars(want)
        assert c[-1] == c[-4] == c[-5] and len(set(c)) < len(c)


def test_more_segments_than_one_step_of_the_capped_grid(ctx):
    """1.25 steps of the DP kernel's grid, and of the waves of the verify and plan kernels, worked out from the device's CU count."""
    inp, p, step = I.many_segments_case(n_cu())
    assert step == n_cu() * M.BLOCKS_PER_CU * (M.THREADS // 64)
    with nt.ChainAlignments(ctx) as al:
        aligned(al, "many segments", inp, p)
        assert al.stats()["n_dp_segments"] == step + step // 4


def test_refusals_leave_the_held_result_unchanged(ctx):
    """One input per flag of the verification, bad parameters and the refusals before any device call: the held result is bit for bit
    what it was.  Then a span of 2^28, refused as unsupported, and of 2^28 - 1, accepted and too long."""
    inp = I.strands_case()[1]
    with nt.ChainAlignments(ctx) as al:
        d = dev_input(inp)
        # on a handle that holds nothing - before any run, and behind a trim - a refused call leaves nothing held
        for again in (False, True):
            what, bad, status = I.refused_cases()[7]
            assert status_of(al.run, *run_args(dev_input(bad)), **kw_of(I.DEFAULT)) == status == M.ERR_BAD_ARG
            assert al.stats() == {**M.EMPTY_STATS, "device_bytes": 0} and al.device_arrays() == (0,) * 6 and al.read()[0].shape == (0, 8), (what, again)
            if not again:
                aligned(al, "before", inp, I.DEFAULT, d)
                al.trim()
        before, _ = aligned(al, "before", inp, I.DEFAULT, d)
        arrays, st = al.device_arrays(), al.stats()

        def unchanged(what):
            assert_result(al.read(), before, what)
            assert al.device_arrays() == arrays and al.stats() == st, what

        for what, bad, status in I.refused_cases():
            assert M.verify(bad, I.DEFAULT) == status
            assert status_of(al.run, *run_args(dev_input(bad)), **kw_of(I.DEFAULT)) == status, what
            unchanged(what)
        lib, h = AL.lib(), al._h
        vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731

        def call(params, t=d, **sizes):
            n = dict(ref_bytes=d[0].numel(), n_refs=d[1].numel() - 1, seq_bytes=d[2].numel(), n_reads=d[3].numel() - 1, n_chains=d[6].numel() - 1,
                     n_members=d[7].numel(), n_anchors=d[8].numel(), n_sel=d[10].numel())
            n.update(sizes)
            p = [x if x is None or isinstance(x, C.c_void_p) else vp(x) for x in t]
            return lib.ntk_align_run_device(h, p[0], n["ref_bytes"], p[1], n["n_refs"], p[2], n["seq_bytes"], p[3], n["n_reads"], p[4], p[5], p[6], p[7],
                                            p[8], p[9], n["n_chains"], n["n_members"], n["n_anchors"], p[10], n["n_sel"], params)
        for p in I.bad_params():
            assert M.check_params(p) == M.ERR_BAD_ARG
            assert call(C.byref(AL.Params(*p))) == M.ERR_BAD_ARG, p
            unchanged(p)
        good = C.byref(AL.Params(*I.DEFAULT))
        assert call(None) == M.ERR_BAD_ARG
        for name in ("n_chains", "n_reads", "n_sel"):
            assert call(good, **{name: 1 << 32}) == M.ERR_BAD_ARG, name
        assert call(good, n_refs=1 << 31) == M.ERR_BAD_ARG
        for i in range(11):
            assert call(good, d[:i] + [None] + d[i + 1:]) == M.ERR_BAD_ARG, i
            if i not in (0, 2):   # (the bytes of a batch lie anywhere)
                assert call(good, d[:i] + [C.c_void_p(d[i].data_ptr() + 2)] + d[i + 1:]) == M.ERR_BAD_ARG, i
        with pytest.raises(ValueError):
            al.run(*run_args(d), 1 << 32)
        unchanged("the host-side refusals")
        for span, status in ((M.SPAN_MAX, M.ERR_UNSUPPORTED), (M.SPAN_MAX - 1, M.OK)):
            far = I.long_span_case(span)
            assert M.verify(far, I.DEFAULT) == status
            assert status_of(al.run, *run_args(dev_input(far)), **kw_of(I.DEFAULT)) == status, span
            if status != M.OK:
                unchanged("a span of 2^28")
        assert al.read()[0].tolist() == [[M.TOO_LONG, 0, 0, 0, 0, 0, 0, 0]] and al.stats()["n_too_long"] == 1


def test_read_capacities(ctx):
    """The size query and NTK_ERR_CAPACITY of read: one capacity for the entries, one for the words; nothing is written."""
    inp, p = I.ties_case()
    with nt.ChainAlignments(ctx) as al:
        want, _ = aligned(al, "ties", inp, p)
        lib, h = AL.lib(), al._h
        n_s, n_c = C.c_uint64(0), C.c_uint64(0)
        assert lib.ntk_align_read(h, None, None, None, None, 0, 0, C.byref(n_s), C.byref(n_c)) == M.ERR_CAPACITY
        ns, nc = want.rows.shape[0], want.cigar.size
        assert (n_s.value, n_c.value) == (ns, nc)
        rows, scores = np.full((ns, 8), 77, dtype=np.uint32), np.full(ns, 77, dtype=np.int64)
        g_offsets, cigar = np.full(ns + 1, 77, dtype=np.uint64), np.full(nc, 77, dtype=np.uint32)
        ptr = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        for cap_s, cap_c in ((ns - 1, nc), (ns, nc - 1)):
            assert lib.ntk_align_read(h, ptr(rows), ptr(scores), ptr(g_offsets), ptr(cigar), cap_s, cap_c, C.byref(n_s), C.byref(n_c)) == M.ERR_CAPACITY
            assert (n_s.value, n_c.value) == (ns, nc) and all((a == 77).all() for a in (rows, scores, g_offsets, cigar))
        assert lib.ntk_align_read(h, ptr(rows), ptr(scores), ptr(g_offsets), ptr(cigar), ns, nc, C.byref(n_s), C.byref(n_c)) == M.OK
        assert_result((rows, scores, g_offsets, cigar), want, "read")
        assert lib.ntk_align_read(h, None, None, None, None, ns, nc, C.byref(n_s), C.byref(n_c)) == M.ERR_BAD_ARG


class _DeviceView:
    def __init__(self, address, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (address, False), "version": 2}


def test_held_memory(ctx):
    """stats.device_bytes is the model's, exactly: after a run, after a smaller run (the arrays stay), after trim (nothing is held) and
    after the run that follows - reuse after growth; result_device is what read returns; a second run replaces the first."""
    large, (small, small_p) = I.seams_case(), I.ties_case()
    with nt.ChainAlignments(ctx) as al:
        want, chains = aligned(al, "seams", large, I.DEFAULT)
        big = M.held(large, I.DEFAULT, want, chains)
        assert al.stats()["device_bytes"] == M.device_bytes(**big), "rocPRIM's temporary storage is not held"
        first, first_chains = aligned(al, "ties", small, small_p)
        assert al.stats()["device_bytes"] == M.device_bytes(**big), "every array keeps the largest size needed so far"
        arrays = al.device_arrays()
        d_rows, d_scores, d_g_offsets, d_cigar, n_s, n_c = arrays
        assert (n_s, n_c) == (first.rows.shape[0], first.cigar.size) and all(arrays[:4])
        clone = lambda a, m, t: torch.as_tensor(_DeviceView(a, m, t), device="cuda").clone().cpu().numpy()   # noqa: E731
        assert np.array_equal(clone(d_rows, n_s * 8, "<i4").view(np.uint32), first.rows.reshape(-1))
        assert np.array_equal(clone(d_scores, n_s, "<i8"), first.scores)
        assert np.array_equal(clone(d_g_offsets, n_s + 1, "<i8").view(np.uint64), first.g_offsets)
        assert np.array_equal(clone(d_cigar, n_c, "<i4").view(np.uint32), first.cigar)
        al.trim()
        assert al.stats() == {**M.EMPTY_STATS, "device_bytes": 0} and al.device_arrays() == (0,) * 6 and al.read()[0].shape == (0, 8)
        aligned(al, "ties", small, small_p)
        assert al.stats()["device_bytes"] == M.device_bytes(**M.held(small, small_p, first, first_chains))
        aligned(al, "seams", large, I.DEFAULT)
        assert al.stats()["device_bytes"] == M.device_bytes(**big), "grown again"
        nothing = I.tiny_cases()["nothing selected"]
        aligned(al, "nothing selected", *nothing)
        assert al.stats()["device_bytes"] == M.device_bytes(**big), "an empty selection keeps the arrays"
    with nt.ChainAlignments(ctx) as al:
        aligned(al, "nothing selected", *nothing)
        assert al.stats()["device_bytes"] == M.device_bytes(0)


# ---- the stream contract ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available(), "these tests need a GPU"
    S.cycles_per_ms()
    r = S.Rig()
    yield r
    r.close()


def test_stream_order(rig):
    """Every call with work pending on the context's stream: the inputs are produced behind the hold (a decoy of the same shape in
    front: other reads, the selection backwards) and clobbered behind the call; read, stats and device_arrays are made with that work
    pending.  run_device, read, stats and trim are SYNC; result_device queues nothing and waits for nothing."""
    inp = I.seams_case()
    decoy = inp._replace(reads=M.pack([I.dna(random.Random(r), M.record_len(inp.reads, r)) for r in range(inp.reads.offsets.size - 1)]),
                         sel=inp.sel[::-1].copy())
    want, _ = model("seams", inp, I.DEFAULT)
    assert M.verify(decoy, I.DEFAULT) == M.OK and not np.array_equal(M.run(decoy, I.DEFAULT)[0].rows, want.rows), "the decoy aligns otherwise"
    inputs = [S.Input(a, b, 0) for a, b in zip(dev_input(inp), dev_input(decoy))]
    with nt.ChainAlignments(rig.ctx) as al:
        def run():
            al.run(*run_args([i.buf for i in inputs]), **kw_of(I.DEFAULT))

        def read():
            arrays = al.device_arrays()
            return al.read(), al.stats(), arrays

        for plain in (True, False):
            _, _, (got, st, arrays) = S.hazard_call(rig, S.SYNC, inputs, [], run, read, plain=plain)
            assert_result(got, want, ("stream order", plain))
            assert st["n_sel"] == len(I.SEAM_SIZES) == arrays[4] and st["n_cigar"] == want.cigar.size == arrays[5]
        S.hazard_call(rig, S.SYNC, [], [], al.read)
        S.hazard_call(rig, S.SYNC, [], [], al.stats)
        S.hazard_call(rig, S.ASYNC, [], [], al.device_arrays)   # with the hold pending: it returns before the stream drains
        S.hazard_call(rig, S.SYNC, [], [], al.trim)             # with a hold pending it has to wait for the stream first
        assert al.stats()["n_sel"] == 0 and al.read()[0].shape == (0, 8)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------

def _device_batch(ctx, records):
    """The records as a device batch and its offsets, laid out by hand: one break byte behind each, 16-byte aligned, padded."""
    b = M.pack(records)
    dev = torch.zeros(b.data.size + 1024, dtype=torch.uint8, device="cuda")
    dev[: b.data.size] = torch.from_numpy(b.data).cuda()
    offs = _wide(b.offsets)
    torch.cuda.synchronize()
    return b, dev, offs


def test_end_to_end_map_aligned(ctx):
    """A 20 kb random reference and 200 reads of 150 to 2000 bases with planted substitutions and indels on both strands through
    ReadMapper.map_aligned: the alignments are the model's on the chains, anchors and selection read back; walking each CIGAR over the
    two intervals finds = on equal bases and X on unequal ones throughout; no chain is too long (the chains' max_dist is below max_seg)."""
    refs, reads = I.sequences()
    k = I.E2E_K
    with nt.ReadMapper(k, I.E2E_W, ctx=ctx) as rm:
        rm.index_records(refs)
        with pytest.raises(ValueError, match="index_records"):
            rm.map_aligned(None, 0, None, 0)
        rb, r_dev, r_offs = _device_batch(ctx, refs)
        qb, q_dev, q_offs = _device_batch(ctx, reads)
        rm.index(r_dev, rb.data.size, r_offs, len(refs))
        got, rows, scores, g_offsets, cigar = rm.map_aligned(q_dev, qb.data.size, q_offs, len(reads), max_dist=I.E2E_MAX_DIST)
        c_offsets, chain_rows, m_offsets, members, _, _, _ = rm.chains.read()
        _, _, _, rpos, qpos, _ = rm.seeds.read()
        _, _, _, out, _ = rm.mappings.read()
        st = rm.alignments.stats()
    inp = M.Input(rb, qb, M.Chains(c_offsets, chain_rows, m_offsets, members, rpos, qpos), out)
    p = M.Params(k)
    want, chains = M.run(inp, p)
    assert_result((rows, scores, g_offsets, cigar), want, "end to end")
    assert {k_: v for k_, v in st.items() if k_ != "device_bytes"} == M.stats(inp, p, want, chains)
    assert st["device_bytes"] == M.device_bytes(**M.held(inp, p, want, chains))
    assert got.size == out.size == rows.shape[0] >= len(reads) and st["n_too_long"] == 0 and st["n_dp_segments"] > 1000
    assert len(set(got["read"].tolist())) == len(reads) and set(got["strand"].tolist()) == {b"+", b"-"}
    ref = refs[0]
    for s, m in enumerate(got):
        read = reads[m["read"]]
        qry = I.revcomp(read) if m["strand"] == b"-" else read
        r, q = int(m["rs"]), (len(read) - int(m["qe"]) if m["strand"] == b"-" else int(m["qs"]))
        for word in cigar[int(g_offsets[s]): int(g_offsets[s + 1])].tolist():
            op, n = word & 15, word >> 4
            if op == M.OP_EQ:
                assert ref[r: r + n] == qry[q: q + n], (s, r, q)
            elif op == M.OP_X:
                assert all(a != b for a, b in zip(ref[r: r + n], qry[q: q + n])), (s, r, q)
            r, q = r + n * (op != M.OP_I), q + n * (op != M.OP_D)
        assert r == m["re"] and q == (len(read) - int(m["qs"]) if m["strand"] == b"-" else int(m["qe"])), s
        assert rows[s, 2] + rows[s, 3] + rows[s, 5] == m["re"] - m["rs"] and rows[s, 2] + rows[s, 3] + rows[s, 4] == m["qe"] - m["qs"], s


# ---- the example program ------------------------------------------------------------------------------------------------------------------

def test_example_program_writes_paf_with_cigars(tmp_path):
    """examples/align_reads on the sequences of the end-to-end test: map_reads' line with n_eq and the alignment's length in columns
    10 and 11, and NM, AS, de and cg behind tp and s1."""
    exe = os.path.join(ROOT, "examples", "align_reads")
    refs, reads = I.sequences()
    reads = reads[:40]
    ref_path, read_path = tmp_path / "refs.fa", tmp_path / "reads.fa"
    ref_path.write_bytes(b"".join(b">ref%d some words\n%s\n" % (i, r) for i, r in enumerate(refs)))
    read_path.write_bytes(b"".join(b">read%d cut\n%s\n" % (q, r) for q, r in enumerate(reads)))
    with nt.ReadMapper(I.E2E_K, I.E2E_W) as rm:
        rb, r_dev, r_offs = _device_batch(rm.ctx, refs)
        qb, q_dev, q_offs = _device_batch(rm.ctx, reads)
        rm.index(r_dev, rb.data.size, r_offs, len(refs))
        got, rows, scores, g_offsets, cigar = rm.map_aligned(q_dev, qb.data.size, q_offs, len(reads))
    want = []
    for s, m in enumerate(got):
        n_eq, n_x, n_ins, n_del = (int(x) for x in rows[s, 2:6])
        nm, cols = n_x + n_ins + n_del, n_eq + n_x + n_ins + n_del
        want.append("read%d\t%d\t%d\t%d\t%s\tref%d\t%d\t%d\t%d\t%d\t%d\t%d\ttp:A:%s\ts1:i:%d\tNM:i:%d\tAS:i:%d\tde:f:%.4f\tcg:Z:%s" % (
            m["read"], len(reads[m["read"]]), m["qs"], m["qe"], m["strand"].decode(), m["ref"], len(refs[m["ref"]]), m["rs"], m["re"], n_eq, cols,
            m["mapq"], "P" if m["primary"] else "S", m["score"], nm, scores[s], nm / cols, nt.cigar_string(cigar[int(g_offsets[s]): int(g_offsets[s + 1])])))
    r = subprocess.run([exe, str(ref_path), str(read_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert len(want) >= len(reads) and r.stdout.splitlines() == want
