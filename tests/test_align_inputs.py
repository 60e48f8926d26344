"""The inputs of tests/test_gpu_align.py (tests/_align_inputs.py) have what they claim, shown with the host model and no GPU: every case
is accepted by the verification; the cases that claim DP segments have them, at the sizes claimed; the band cases' paths touch the edge
they name; the max_seg case has its too-long chains; the groups case takes two groups in 16 MiB; every refused case is refused by
the model for its own reason; the end-to-end sequences make chains none of which is too long."""
import numpy as np

import _align_inputs as I
import _align_model as M


def dp_segments(chains):
    return [s for g in chains for s in g.segments if s is not None]


def test_tiny_cases_are_what_they_say():
    t = I.tiny_cases()
    for name, (inp, p) in t.items():
        assert M.verify(inp, p) == M.OK, name
    runs = {name: M.run(inp, p) for name, (inp, p) in t.items()}
    assert runs["nothing selected"][0].rows.shape == (0, 8) and runs["nothing selected"][0].g_offsets.tolist() == [0]
    assert [len(g.segments) for g in runs["one member"][1]] == [0, 0] and runs["one member"][0].rows[:, 1].tolist() == [1, 3]
    assert not dp_segments(runs["pure gap runs"][1]) and runs["pure gap runs"][0].rows[:, 4:7].tolist() == [[0, 5, 1], [2, 0, 1], [0, 0, 0], [1, 0, 1], [0, 2, 1]]
    assert [(s.n, s.m) for s in dp_segments(runs["one by one"][1])] == [(1, 1)] * 4
    inp, p = t["overlapping anchors"]
    assert M.steps(inp.chains, 0) == [(3, 5), (5, 3)] == M.steps(inp.chains, 1) and I.K == 7 and not dp_segments(runs["overlapping anchors"][1])
    assert int(inp.chains.chain_rows[1, 2]) & 1 == 1


def test_seams_have_the_sizes_and_both_strands():
    inp = I.seams_case()
    _, chains = M.run(inp, I.DEFAULT)
    assert [(s.n, s.m) for s in dp_segments(chains)] == list(I.SEAM_SIZES)
    assert {(63, 63), (64, 64), (65, 65), (127, 127), (128, 128), (129, 129)} <= set(I.SEAM_SIZES)
    assert any(n < 64 < m for n, m in I.SEAM_SIZES) and any(m < 64 < n for n, m in I.SEAM_SIZES)
    assert set((inp.chains.chain_rows[:, 2] & 1).tolist()) == {0, 1}
    assert all(any(op in (M.OP_I, M.OP_D) for op, _ in s.runs) for s in dp_segments(chains) if s.n > 60 and s.m > 60)


def test_band_cases_touch_the_edges_they_name():
    for name, (inp, p, claim) in I.band_cases().items():
        assert M.verify(inp, p) == M.OK
        segs = dp_segments(M.run(inp, p)[1])
        assert segs and all(s.in_band for s in segs), name
        if claim == "lo":
            assert all(s.touches_lo and not s.touches_hi for s in segs) and p.band_pad == 6
        elif claim == "hi":
            assert all(s.touches_hi and not s.touches_lo for s in segs) and p.band_pad == 6
        elif claim == "wide":
            assert all(p.band_pad > max(s.n, s.m) and not s.touches_lo and not s.touches_hi for s in segs)
        elif claim == "pair":
            free = dp_segments(M.run(inp, p._replace(band_pad=64))[1])
            assert p.band_pad == 0 and all(s.n == s.m for s in segs)
            assert all({M.OP_I, M.OP_D} <= {op for op, _ in f.runs} and f.score > s.score and not {M.OP_I, M.OP_D} & {op for op, _ in s.runs}
                       for s, f in zip(segs, free))
        else:
            assert p.band_pad == 0 and all(s.n != s.m for s in segs)


def test_ties_bases_strands_and_selection():
    inp, p = I.ties_case()
    want, chains = M.run(inp, p)
    assert any({M.OP_I, M.OP_D} <= {op for op, _ in s.runs} for s in dp_segments(chains)) and p.b == 255
    inp = I.bases_case()
    assert M.verify(inp, I.DEFAULT) == M.OK
    assert {ord("N"), ord("\n"), ord("a"), ord("U"), ord("u")} <= set(inp.refs.data.tolist()) | set(inp.reads.data.tolist())
    for inp in I.strands_case()[:1]:
        ch = inp.chains
        for c in range(2):
            m = M.members_of(ch, c)
            q = (int(ch.qpos[m[0]]), int(ch.qpos[m[-1]]))
            assert int(ch.rpos[m[0]]) == 0 and int(ch.rpos[m[-1]]) + I.K == M.record_len(inp.refs, c) and min(q) == 0 and max(q) + I.K == M.record_len(inp.reads, c)
        assert (ch.chain_rows[:, 2] & 1).tolist() == [0, 1] and len(dp_segments(M.run(inp, I.DEFAULT)[1])) == 4
    sel = I.selection_case().sel.tolist()
    assert len(set(sel)) < len(sel) and sel != sorted(sel) and set(range(len(I.SEAM_SIZES))) - set(sel)


def test_max_seg_and_largest():
    inp, p, too_long = I.max_seg_case()
    want, chains = M.run(inp, p)
    assert [i for i, g in enumerate(chains) if g.too_long] == too_long
    at = [max(max(part[3], part[4]) for part in M.parts_of(inp, c, p) if part[0] == "between") for c in inp.sel.tolist()]
    assert at == [p.max_seg, p.max_seg + 1, p.max_seg, p.max_seg + 1, p.max_seg + 1, p.max_seg + 1]
    inp, p = I.largest_case()
    sizes = [(part[3], part[4]) for c in range(3) for part in M.parts_of(inp, c, p) if part[0] == "between"]
    assert sizes == [(100, 100), (4095, 4095), (100, 100)] and p.band_pad == 4095 == M.SEG_MAX
    assert sizes[1][0] * min(2 * p.band_pad + 1, sizes[1][1]) <= 16 << 20, "the largest part fits the smallest workspace"
    inp, p = I.groups_case()
    sizes = [(part[3], part[4]) for c in range(3) for part in M.parts_of(inp, c, p) if part[0] == "between"]
    bytes_ = [n * min(2 * p.band_pad + 1, m) for n, m in sizes]
    assert sizes == [(I.GROUP_PART,) * 2] * 3 and sum(bytes_) > 16 << 20 > sum(bytes_[:2])
    assert [g[:2] for g in M.groups(bytes_, 16 << 20)] == [(0, 2), (2, 3)] and len(M.groups(bytes_, 256 << 20)) == 1


def test_many_segments_pass_one_step_of_the_grid():
    inp, p, step = I.many_segments_case(4)
    assert step == 4 * 8 * 4 and inp.sel.size == step + step // 4 and M.verify(inp, p) == M.OK
    assert all((part[3], part[4]) == (1, 1) for c in range(5) for part in M.parts_of(inp, c, p) if part[0] == "between")


def test_refused_cases_are_refused_one_flag_each():
    good = I.strands_case()[1]
    assert M.verify(good, I.DEFAULT) == M.OK
    cases = I.refused_cases()
    assert len(cases) == 15 and len({what for what, _, _ in cases}) == 15
    for what, bad, status in cases:
        assert M.verify(bad, I.DEFAULT) == status == M.ERR_BAD_ARG, what


def test_end_to_end_sequences():
    """The references and reads of the end-to-end test: one reference of 20 kb, 200 reads of about 150 to 2000 bases, half of them
    reverse-complemented, each carrying planted errors.  No chain of them can be too long: consecutive members of a chain lie at most
    max_dist apart on both sequences (the chain library's rule), so n, m <= max_dist, and the test chains with a max_dist below the
    default max_seg."""
    assert I.E2E_MAX_DIST <= M.Params(I.E2E_K).max_seg == 2048
    # the chain library's rule, from its own model (tests/_chain_model.py, which tests/test_gpu_chain.py holds the library to): a pair
    # of anchors is chained only where 1 <= dr <= max_dist and 1 <= dq <= max_dist, on both strands ...
    import _chain_model as CM
    cp, d = CM.Params(I.E2E_K, max_dist=I.E2E_MAX_DIST), I.E2E_MAX_DIST
    for rev in (0, 1):
        q = lambda step: 5000 - step if rev else 5000 + step   # noqa: E731
        assert CM.pair(rev, 100, 5000, 100 + d, q(d), cp) is not None
        assert CM.pair(rev, 100, 5000, 100 + d + 1, q(d + 1), cp) is None
        assert CM.pair(rev, 100, 5000, 100 + d + 1, q(d), cp) is None and CM.pair(rev, 100, 5000, 100 + d, q(d + 1), cp) is None
    # ... so anchors that lie max_dist + 1 apart end one chain and begin another, and every between part of a chain has n, m <= max_dist
    run = [(0, 100 + 10 * i, 10 * i) for i in range(5)]
    far = [(0, r + 40 + d + 1, p + 40 + d + 1) for _, r, p in run]
    anchors = CM.one_read(run + far)
    got = CM.chain(anchors, cp)
    assert got.chain_rows.shape[0] == 2 and got.m_offsets.tolist() == [0, 5, 10]
    for c in range(2):
        m = got.members[int(got.m_offsets[c]): int(got.m_offsets[c + 1])].tolist()
        assert all(1 <= int(anchors[2][i]) - int(anchors[2][j]) <= d and 1 <= int(anchors[3][i]) - int(anchors[3][j]) <= d for j, i in zip(m, m[1:]))
    refs, reads = I.sequences()
    assert [len(r) for r in refs] == [20000] and len(reads) == 200 and min(len(r) for r in reads) >= 130 and max(len(r) for r in reads) <= 2200
    assert sum(r in refs[0] for r in reads) < 10 and sum(I.revcomp(r) in refs[0] for r in reads) < 10, "the reads carry errors"
    assert np.frombuffer(I.revcomp(b"ACGTN"), dtype=np.uint8).tobytes() == b"NACGT"
