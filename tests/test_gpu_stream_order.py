"""Every device-face call of tests/_stream_contract.py held to its stream contract while the context's stream is busy, on a real MI355X.

The context works on a non-blocking torch side stream; every input is produced on that stream behind a bounded spin, every output is
poisoned on it, the call is made while both are pending, the inputs are overwritten behind it and the outputs are consumed by clones on
the stream (tests/_stream_order.py `hazard_call`).  Each case asserts its own preconditions: the producer was pending when the call was
made, it was still pending when an ASYNC call returned, and the stream was drained when a SYNC call returned.  Every handle first makes
the same call the plain way (the warm-up, compared as well), so the hazard run allocates nothing.  Truth is the host models;
tests/test_stream_order_inputs.py proves on the CPU that the decoy, the clobber and a skipped stage each give another answer.

Calls go through the ctypes entries wherever the facade method synchronises the device itself (that would drain the hold).  The hold is
the larger of 20 ms and ten times the longest host-side return time of an ASYNC call measured so far in the session (each ASYNC case
times its own call on the warm handle and an idle stream before its hazard run); profiles/stream_order/README.md has the numbers."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
import oracle as O  # noqa: E402
from needletail_amd import _lib as NL  # noqa: E402
from needletail_amd import dbg as dbg_lib, kmer_sets as ks_lib  # noqa: E402

import _stream_order as S  # noqa: E402
from _stream_order import ASYNC, BYTES, CUTOFF, MAY_SYNC, NORMALIZE, SYNC, ptr  # noqa: E402

pytestmark = pytest.mark.gpu

u64 = C.c_uint64
CAPACITY = 1 << 15   # of every table and index here: above the distinct k-mers of any batch of the file
RETURNS = {}         # ASYNC case -> host-side return time of its call, ms


@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available(), "these tests need a GPU"
    S.cycles_per_ms()
    r = S.Rig()
    yield r
    print(f"stream_order: {r.queued_ms:.0f} ms of hold queued by the shared rig; return times (ms) "
          f"{({k: round(v, 3) for k, v in RETURNS.items()})}; hold at the end {S.hold_ms():.1f} ms")
    r.ctx.set_option(NL.OPT_MINIMIZER_ROUTE, 0)
    r.close()


def run(rig, name, kind, inputs, outputs, call, check, read=None):
    """The warm-up, for an ASYNC call a timed repeat of it that sizes the hold, then the hazard run; all held to the model by `check`."""
    result = S.hazard_call(rig, kind, inputs, outputs, call, read, plain=True)
    check(*result, (name, "warm-up"))
    if kind == ASYNC:
        box = {}

        def timed_call():
            rig.side.synchronize()
            import time
            t0 = time.perf_counter()
            out = call()
            box["ms"] = (time.perf_counter() - t0) * 1e3
            return out
        result = S.hazard_call(rig, kind, inputs, outputs, timed_call, read, plain=True)
        check(*result, (name, "timed repeat"))
        RETURNS[name] = box["ms"]
        S.set_hold_ms(RETURNS)
    result = S.hazard_call(rig, kind, inputs, outputs, call, read, plain=False)
    check(*result, (name, "hazard"))


def batch_inputs(k, lower=False, repeat=False, quality=False, offsets=False):
    t, d = S.batches(k, lower, repeat)
    seq = S.batch_input(t.buf, d.buf)
    qual = S.Input(S.dev_bytes(t.qual.tobytes(), fill=0xFF), S.dev_bytes(d.qual.tobytes(), fill=0xFF), 0) if quality else None
    off = S.words_input(t.offsets, np.zeros_like(t.offsets), 0) if offsets else None
    return t, d, seq, qual, off


def some(*inputs):
    return [i for i in inputs if i is not None]


def acc_stats(words: np.ndarray) -> dict:
    """The accumulator words of a bound buffer as the oracle's stats."""
    return {"n_total": int(words[NL.ACC_N_TOTAL]), "n_fwd": int(words[NL.ACC_N_FWD]), "n_rc": int(words[NL.ACC_N_RC]),
            "sum": int(words[NL.ACC_SUM]), "xor": int(words[NL.ACC_XOR]), "hist": words[NL.ACC_HIST:NL.ACC_HIST + NL.HIST_BINS].copy()}


class bound_accumulator:
    """The context accumulates into a tensor of the test's own: the consumer is its clone on the stream, and NTK_ACC_REDONE says which
    kernel's result a speculative launch took."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.acc = torch.zeros(NL.ACC_WORDS, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def __enter__(self):
        self.ctx.accum_bind_device(self.acc)
        return self.acc

    def __exit__(self, *exc):
        self.ctx.accum_bind_device(None)


# ---- the core, ASYNC ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case_id", S.REDUCE_IDS)
def test_reduce_device(rig, case_id):
    """ntk_reduce_device / ntk_reduce_device_quality on the four routes: the packed-value scan, the 2-bit path, the speculative pair with
    its redo taken (one lower-case base in input that was not normalised), and the k > 32 packed-stream kernel with its byte-walking redo
    (the lower-case base again: at k = 47 no k-mer can tie with its reverse complement over 32 bases, the inverted repeat is there all the
    same).  ntk_accum_reset is queued ahead, inside the call; ntk_accum_read after the clobber and a clone of the bound accumulator are
    the consumers."""
    route, quality = case_id.rsplit("-", 1)
    k, path, pre, lower, repeat = S.REDUCE_ROUTES[route]
    quality = quality == "quality"
    want = S.CASES[f"reduce-{case_id}"].truth()
    t, d, seq, qual, _ = batch_inputs(k, lower, repeat, quality)
    ctx = rig.ctx

    def call():
        ctx.accum_reset()
        ctx.reduce_device(seq.buf, t.n, k, path, pre, d_qual=qual.buf if quality else None, quality_cutoff=CUTOFF if quality else 0)

    def check(_, clones, got, what):
        S.assert_answer(got, want, what)
        words = S.host(clones[0])
        S.assert_answer(acc_stats(words), want, (what, "the bound accumulator's clone"))
        assert int(words[NL.ACC_REDONE]) == (1 if lower else 0), (what, "launches redone", int(words[NL.ACC_REDONE]))
        assert got["n_undigested"] == (got["n_total"] if k > 32 else 0), what

    with bound_accumulator(ctx) as acc:
        run(rig, f"reduce-{case_id}", ASYNC, some(seq, qual), [acc], call, check, read=ctx.accum_read)


def _decoy_reduce_then(rig, name, tail):
    """A reduce of the (complete) decoy batch queued ahead of `tail(seq, n)`, which must start a new result on the stream."""
    want = S.CASES[name].truth()
    t, d, seq, _, _ = batch_inputs(21)
    ahead = S.dev_bytes(d.buf)
    ctx = rig.ctx

    def call():
        ctx.reduce_device(ahead, d.n, 21, BYTES, NORMALIZE)
        tail(seq.buf, t.n)

    run(rig, name, ASYNC, [seq], [], call, lambda _, __, got, what: S.assert_answer(got, want, what), read=ctx.accum_read)


def test_reduce_with_the_reset_flag(rig):
    """NTK_FLAG_RESET with the accumulators loaded, on the stream, by a reduce of the decoy: the zeroing folded into the launch lands
    between the two reduces, not ahead of both."""
    _decoy_reduce_then(rig, "reset_flag", lambda seq, n: rig.ctx.reduce_device(seq, n, 21, BYTES, NORMALIZE, reset=True))


def test_accum_reset_ahead_of_a_reduce(rig):
    def tail(seq, n):
        rig.ctx.accum_reset()
        rig.ctx.reduce_device(seq, n, 21, BYTES, NORMALIZE)
    _decoy_reduce_then(rig, "accum_reset", tail)


def test_accum_bind_device(rig):
    """Bound to a torch tensor inside the call; the tensor is cloned on the stream and never read through ntk_accum_read."""
    want = S.CASES["accum_bind"].truth()
    t, d, seq, _, _ = batch_inputs(21)
    ctx = rig.ctx
    acc = torch.zeros(NL.ACC_WORDS, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def call():
        ctx.accum_bind_device(acc)
        assert ctx.accum_device_ptr() == acc.data_ptr()   # (ntk_accum_device_ptr: the host's view of the binding, no stream work)
        ctx.accum_reset()
        ctx.reduce_device(seq.buf, t.n, 21, BYTES, NORMALIZE)
        ctx.accum_bind_device(None)
        assert ctx.accum_device_ptr() != acc.data_ptr()

    try:
        run(rig, "accum_bind", ASYNC, [seq], [acc], call, lambda _, clones, __, what: S.assert_answer(acc_stats(S.host(clones[0])), want, what))
    finally:
        ctx.accum_bind_device(None)


@pytest.mark.parametrize("route", list(S.MINIMIZER_ROUTES))
def test_minimizers_reduce_device(rig, route):
    k, w, off = S.MINIMIZER_ROUTES[route]
    want = S.CASES[f"minimizers-{route}"].truth()
    t, d, seq, _, _ = batch_inputs(k)
    ctx = rig.ctx

    def call():
        ctx.accum_reset()
        ctx.minimizers_reduce_device(seq.buf, t.n, k, w, BYTES, NORMALIZE)

    ctx.set_option(NL.OPT_MINIMIZER_ROUTE, off)
    try:
        run(rig, f"minimizers-{route}", ASYNC, [seq], [], call, lambda _, __, got, what: S.assert_answer(got, want, what), read=ctx.accum_read)
    finally:
        ctx.set_option(NL.OPT_MINIMIZER_ROUTE, 0)


def unpack_plane(t, n: int) -> np.ndarray:
    """Bit (15 - e % 16) of word e / 16, for e < n."""
    w = t.cpu().numpy().view(np.uint16)
    return ((w[:, None] >> (15 - np.arange(16, dtype=np.uint16))[None, :]) & 1).reshape(-1)[:n].astype(bool)


@pytest.mark.parametrize("case_id", S.MATERIALIZE_IDS)
def test_materialize_device(rig, case_id):
    """The three planes, consumed by clones."""
    route, quality = case_id.rsplit("-", 1)
    k, path, pre = S.MATERIALIZE_ROUTES[route]
    quality = quality == "quality"
    want = S.CASES[f"materialize-{case_id}"].truth()
    t, d, seq, qual, _ = batch_inputs(k, quality=quality)
    padded = (t.n + 15) // 16 * 16
    values = torch.zeros(padded, dtype=torch.int64, device="cuda")
    valid16, rc16 = torch.zeros(padded // 16, dtype=torch.int16, device="cuda"), torch.zeros(padded // 16, dtype=torch.int16, device="cuda")
    ctx = rig.ctx

    def call():
        if quality:   # (the facade always enters through ntk_materialize_device_quality: the plain entry is called by name)
            ctx.materialize_device(seq.buf, t.n, k, path, pre, values, valid16, rc16, d_qual=qual.buf, quality_cutoff=CUTOFF)
        else:
            p = params(k, path, pre)
            NL.check(NL.lib().ntk_materialize_device(ctx._h, ptr(seq.buf), t.n, C.byref(p), ptr(values), ptr(valid16), ptr(rc16)), "ntk_materialize_device")

    def check(_, clones, __, what):
        valid = unpack_plane(clones[1], t.n)
        got = {"valid": valid, "rc": unpack_plane(clones[2], t.n) & valid, "values": np.where(valid, S.host(clones[0])[:t.n], np.uint64(0))}
        S.assert_answer(got, want, what)

    run(rig, f"materialize-{case_id}", ASYNC, some(seq, qual), [values, valid16, rc16], call, check)


def test_reverse_complement_records_device(rig):
    n_records, record_len, stride = S.RC_RECORDS
    want = S.CASES["rc_records"].truth()["out"]
    src = S.batch_input(S.stride_records(0), S.stride_records(1))
    out = torch.zeros_like(src.buf)
    n = n_records * stride

    def call():
        rig.ctx.reverse_complement_records_device(src.buf, out, n_records, record_len, stride)

    run(rig, "rc_records", ASYNC, [src], [out], call, lambda _, clones, __, what: S.assert_answer({"out": S.host(clones[0])[:n]}, {"out": want}, what))


def test_synth_reads_device_into_a_reduce(rig):
    """The generator's output consumed by a reduce queued straight behind it."""
    seed, first, n_reads, read_len, n_per_1024 = S.SYNTH
    want = S.CASES["synth_into_reduce"].truth()
    reads = O.synth_reads(*S.SYNTH)
    n = n_reads * (read_len + 1)
    out = torch.zeros((n + 15) // 16 * 16 + 64, dtype=torch.uint8, device="cuda")
    ctx = rig.ctx

    def call():
        ctx.synth_reads_device(seed, first, n_reads, read_len, n_per_1024, out)
        ctx.accum_reset()
        ctx.reduce_device(out, n, 21, BYTES, NORMALIZE)

    def check(_, clones, got, what):
        assert np.array_equal(S.host(clones[0])[:n], reads), what
        S.assert_answer(got, want, what)

    run(rig, "synth_into_reduce", ASYNC, [], [out], call, check, read=ctx.accum_read)


def test_batch_submit_behind_pending_work(rig):
    """A pinned batch submitted while the hold, a reduce of the decoy and an ntk_accum_reset are pending on the context's stream: the copy
    streams run ahead, the scan must not.  After the wait the result is that of the batch alone."""
    want = S.CASES["batch_submit"].truth()
    t, d = S.batches(21)
    ahead = S.dev_bytes(d.buf)
    ctx = rig.ctx
    bt = ctx.batch(1 << 16, 1024)

    def call():
        for r in t.records:
            assert bt.append(r, NORMALIZE)
        ctx.reduce_device(ahead, d.n, 21, BYTES, NORMALIZE)
        ctx.accum_reset()
        bt.submit(21, BYTES, NORMALIZE)

    def read():
        bt.wait()
        return ctx.accum_read()

    try:
        run(rig, "batch_submit", ASYNC, [], [], call, lambda _, __, got, what: S.assert_answer(got, want, what), read=read)
    finally:
        bt.release()


def test_two_reduces_and_the_partials_grow():
    """Two reduces back to back behind one hold on a context that has only seen the small batch: the second needs more partial rows
    (tests/_stream_order.py GROW_READS says how many, from the launch plan), so ensure_partials replaces the arrays the first one, still
    queued, writes - THE ONE RULE of ntk_device_mem.hpp.  The first call returns at once; the second may wait.  The sum is that of both."""
    want = S.CASES["two_reduces_partials_grow"].truth()
    t, d, seq, _, _ = batch_inputs(21)
    big = O.synth_reads(*S.GROW_READS).tobytes()
    d_big = S.dev_bytes(big)
    rig = S.Rig()
    ctx = rig.ctx
    try:
        def small():
            ctx.accum_reset()
            ctx.reduce_device(seq.buf, t.n, 21, BYTES, NORMALIZE)

        _, _, got = S.hazard_call(rig, ASYNC, [seq], [], small, ctx.accum_read, plain=True)
        S.assert_answer(got, S.reduce_answer(t.buf, 21, BYTES, NORMALIZE), "warm-up")
        pending = {}

        def both():
            small()
            pending["after the first"] = not rig.ev_in.query()
            ctx.reduce_device(d_big, len(big), 21, BYTES, NORMALIZE)

        _, _, got = S.hazard_call(rig, MAY_SYNC, [seq], [], both, ctx.accum_read)
        assert pending["after the first"], "the first reduce returned after its input was produced"
        S.assert_answer(got, want, "hazard")
    finally:
        rig.close()


def test_a_context_that_owns_its_stream():
    """nt.Context(0): the stream is the context's own, wrapped for torch from ntk_ctx_stream's pointer."""
    want = S.CASES["own_stream"].truth()
    t, d, seq, _, _ = batch_inputs(21)
    rig = S.Rig(own_stream=True)
    ctx = rig.ctx
    try:
        def call():
            ctx.accum_reset()
            ctx.reduce_device(seq.buf, t.n, 21, BYTES, NORMALIZE)
        run(rig, "own_stream", ASYNC, [seq], [], call, lambda _, __, got, what: S.assert_answer(got, want, what), read=ctx.accum_read)
    finally:
        rig.close()


# ---- the libraries, ASYNC -------------------------------------------------------------------------------------------------------------------

class TableReader:
    """The reading calls of a count table's header, made on the stream behind the counting: stats, extract, spectrum and lookup."""

    def __init__(self, table, k, path, pre):
        q = S.table_queries(k, path, pre)
        self.table, self.n = table, q.shape[0]
        self.d_q, self.d_c = S.dev_words(q), torch.zeros(q.shape[0], dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()

    def __call__(self):
        t = self.table
        st, (keys, counts) = t.stats(), t.items()
        t._check("lookup_device", t._h, ptr(self.d_q), self.n, ptr(self.d_c))
        return {"keys": keys, "counts": counts, "n_distinct": st["n_distinct"], "n_total": st["n_total"], "spectrum": t.spectrum(64),
                "n_dropped": st["n_dropped"], "lookup": S.host(self.d_c)}


def check_table(want):
    def check(_, __, got, what):
        S.assert_answer(got, want, what)
        assert got["n_dropped"] == 0, what
    return check


@pytest.mark.parametrize("which", list(S.TABLES))
def test_count_table(rig, which):
    """count_device of the decoy, ntk_kmer_table_reset / ntk_wide_table_reset and count_device of the batch, all queued; stats, extract and
    spectrum follow with no host wait in between: they synchronise and must see all of it."""
    k, path, pre = S.TABLES[which]
    want = S.CASES[f"count_table-{which}"].truth()
    t, d, seq, _, _ = batch_inputs(k)
    ahead = S.dev_bytes(d.buf)
    with (nt.KmerTable if which == "narrow" else nt.WideKmerTable)(k, path, CAPACITY, rig.ctx) as table:
        def call():
            table.count_device(ahead, d.n, pre)
            table.reset()
            table.count_device(seq.buf, t.n, pre)
        run(rig, f"count_table-{which}", ASYNC, [seq], [], call, check_table(want), read=TableReader(table, k, path, pre))


def _scratch_grows(rig, name, handle, add, read, small_answer):
    """A second, larger batch queued while the first is pending on a handle that has only seen the small one: MaterialiseScratch.ensure
    (ntk_consumer.hpp, grow_exact) must replace the three arrays the first call's kernels, still queued, read."""
    want = S.CASES[name].truth()
    t, d, seq, _, _ = batch_inputs(21)
    big = O.synth_reads(*S.GROW_COUNT_READS).tobytes()
    assert (len(big) + 15) // 16 > (t.n + 15) // 16, "the larger batch needs a longer scratch (one chunk each: both are far below 64 Mi bases)"
    d_big = S.dev_bytes(big)

    def small():
        handle.reset()
        add(seq.buf, t.n)

    _, _, got = S.hazard_call(rig, ASYNC, [seq], [], small, read, plain=True)
    S.assert_answer(got, small_answer(t.buf), (name, "warm-up"))
    pending = {}

    def both():
        small()
        pending["after the first"] = not rig.ev_in.query()
        add(d_big, len(big))

    _, _, got = S.hazard_call(rig, MAY_SYNC, [seq], [], both, read)
    assert pending["after the first"], "the first call returned after its input was produced"
    S.assert_answer(got, want, (name, "hazard"))


def test_count_table_scratch_grows(rig):
    with nt.KmerTable(21, BYTES, CAPACITY, rig.ctx) as table:
        _scratch_grows(rig, "count_table_scratch_grows", table, lambda seq, n: table.count_device(seq, n, NORMALIZE), TableReader(table, 21, BYTES, NORMALIZE),
                       lambda buf: S._table_answer(21, BYTES, NORMALIZE, buf))


def read_sketch(sk):
    return {"registers": sk.registers(), "n_windows": sk.estimate()["n_windows"]}


def test_kmer_sketch(rig):
    """add_device of the decoy, ntk_kmer_sketch_reset, add_device of the batch; registers and estimate synchronise."""
    want = S.CASES["kmer_sketch"].truth()
    t, d, seq, _, _ = batch_inputs(21)
    ahead = S.dev_bytes(d.buf)
    with nt.KmerSketch(21, BYTES, rig.ctx) as sk:
        def call():
            sk.add_device(ahead, d.n, NORMALIZE)
            sk.reset()
            sk.add_device(seq.buf, t.n, NORMALIZE)
        run(rig, "kmer_sketch", ASYNC, [seq], [], call, lambda _, __, got, what: S.assert_answer(got, want, what), read=lambda: read_sketch(sk))


def test_kmer_sketch_scratch_grows(rig):
    with nt.KmerSketch(21, BYTES, rig.ctx) as sk:
        _scratch_grows(rig, "kmer_sketch_scratch_grows", sk, lambda seq, n: sk.add_device(seq, n, NORMALIZE), lambda: read_sketch(sk),
                       lambda buf: S._sketch_answer(21, BYTES, NORMALIZE, buf))


def test_kmer_colors_add(rig):
    """The decoy's list queued under colour 0, ntk_kmer_colors_reset, then the list under one mask and per-key masks for every other key;
    lookup_device and stats follow on the stream."""
    want = S.CASES["colors_add"].truth()
    (kt, st, mt), (kd, sd, md) = S.color_lists("true"), S.color_lists("decoy")
    keys, sub, masks = S.words_input(kt, kd), S.words_input(st, sd), S.words_input(mt, md)
    ahead = S.dev_words(kd)
    queries = S.color_queries()
    d_q = S.dev_words(queries)
    d_m = torch.zeros(queries.size, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with nt.KmerColors(21, BYTES, S.N_COLORS, CAPACITY, rig.ctx) as kc:
        def call():
            kc._check("add_device", kc._h, ptr(ahead), None, 1, kd.size)
            kc.reset()
            kc._check("add_device", kc._h, ptr(keys.buf), None, 1, kt.size)
            kc._check("add_device", kc._h, ptr(sub.buf), ptr(masks.buf), 0, st.size)

        def read():
            kc._check("lookup_device", kc._h, ptr(d_q), queries.size, ptr(d_m))
            st_ = kc.stats()
            return {"lookup": S.host(d_m), "n_keys": st_["n_keys"], "n_masked_bits": st_["n_masked_bits"], "per_color": st_["per_color"],
                    "n_dropped": st_["n_dropped"]}

        def check(_, __, got, what):
            S.assert_answer(got, want, what)
            assert got["n_dropped"] == 0, what

        run(rig, "colors_add", ASYNC, [keys, sub, masks], [], call, check, read=read)


# ---- the libraries, MAY_SYNC and SYNC ---------------------------------------------------------------------------------------------------------

def test_minhash_add_device(rig):
    """ntk_minhash_reset and ntk_minhash_add_device on a handle that holds the decoy's k-mers, then read and stats."""
    want = S.CASES["minhash"].truth()
    t, d, seq, _, _ = batch_inputs(21)
    ahead = S.dev_bytes(d.buf)
    ctx = rig.ctx
    with nt.KmerMinHash(21, BYTES, ctx=ctx, **S.MINHASH) as mh:
        def call():
            mh.reset()
            mh.add_device(seq.buf, t.n, NORMALIZE)

        def read():
            (h, c), st = mh.hashes(), mh.stats()
            return {"hashes": h, "counts": c, "n_windows": st["n_windows"]}

        for plain in (True, False):
            mh.add_device(ahead, d.n, NORMALIZE)   # the handle holds something the reset has to remove
            ctx.synchronize()
            _, _, got = S.hazard_call(rig, MAY_SYNC, [seq], [], call, read, plain=plain)
            S.assert_answer(got, want, ("minhash", plain))


def params(k, path, pre, cutoff=0):
    return NL.Params(k, path, pre, NL.flags(0, cutoff))


def test_read_abundance(rig):
    """The table is reset and counts the batch on the stream; ntk_read_abundance_run_device follows in the same chain with no wait in
    between, its batch, quality stream and offsets produced behind the hold."""
    want = S.CASES["read_abundance"].truth()
    t, d, seq, qual, off = batch_inputs(21, quality=True, offsets=True)
    rows = torch.zeros((S.N_RECORDS, 6), dtype=torch.int64, device="cuda")
    p = params(21, BYTES, NORMALIZE, CUTOFF)
    with nt.KmerTable(21, BYTES, CAPACITY, rig.ctx) as table, nt.ReadAbundance(table) as ra:
        def call():
            table.reset()
            table.count_device(seq.buf, t.n, NORMALIZE)
            ra._check("run_device", ra._h, ptr(seq.buf), ptr(qual.buf), t.n, ptr(off.buf), S.N_RECORDS, C.byref(p), S.ABUNDANCE_MIN_COUNT, ptr(rows))
        run(rig, "read_abundance", SYNC, [seq, qual, off], [rows], call, lambda _, clones, __, what: S.assert_answer({"rows": S.host(clones[0])}, want, what))


class TrimBuffers:
    """The outputs of ntk_read_trim_run_device and ntk_read_trim_compact_device for a batch of n bytes and n_records records."""

    def __init__(self, n, n_records):
        self.cap = (n + 15) // 16 * 16
        self.rows = torch.zeros((n_records, 4), dtype=torch.int64, device="cuda")
        self.seq, self.aux = torch.zeros(self.cap + 64, dtype=torch.uint8, device="cuda"), torch.zeros(self.cap + 64, dtype=torch.uint8, device="cuda")
        self.offsets, self.source = torch.zeros(n_records + 1, dtype=torch.int64, device="cuda"), torch.zeros(n_records, dtype=torch.int64, device="cuda")
        self.n_records = n_records

    def all(self):
        return [self.rows, self.seq, self.aux, self.offsets, self.source]


def trim_and_compact(rt, p, seq, qual, n, off, b: TrimBuffers):
    rt._check("run_device", rt._h, ptr(seq), ptr(qual), n, ptr(off), b.n_records, C.byref(p), S.TRIM["min_count"], S.TRIM["mode"],
              S.TRIM["min_length"], ptr(b.rows))
    nb, nr = u64(0), u64(0)
    rt._check("compact_device", rt._h, ptr(seq), ptr(qual), n, ptr(off), b.n_records, ptr(b.rows), ptr(b.seq), ptr(b.aux), b.cap,
              ptr(b.offsets), ptr(b.source), b.n_records, C.byref(nb), C.byref(nr))
    return int(nb.value), int(nr.value)


def trim_answer_of(result, clones):
    nb, nr = result
    pad = (nb + 15) // 16 * 16
    return {"rows": S.host(clones[0]), "n_bytes": nb, "seq": S.host(clones[1])[:pad], "aux": S.host(clones[2])[:pad],
            "offsets": S.host(clones[3])[:nr + 1], "source": S.host(clones[4])[:nr]}


def test_read_trim_and_compact(rig):
    """ntk_read_trim_run_device and ntk_read_trim_compact_device behind the table's reset and count, all in one chain."""
    want = S.CASES["read_trim"].truth()
    t, d, seq, qual, off = batch_inputs(21, quality=True, offsets=True)
    b = TrimBuffers(t.n, S.N_RECORDS)
    p = params(21, BYTES, NORMALIZE, CUTOFF)
    with nt.KmerTable(21, BYTES, CAPACITY, rig.ctx) as table, nt.ReadTrimmer(table) as rt:
        def call():
            table.reset()
            table.count_device(seq.buf, t.n, NORMALIZE)
            return trim_and_compact(rt, p, seq.buf, qual.buf, t.n, off.buf, b)
        run(rig, "read_trim", SYNC, [seq, qual, off], b.all(), call, lambda result, clones, __, what: S.assert_answer(trim_answer_of(result, clones), want, what))


def test_record_minhash(rig):
    """ntk_record_minhash_run_device reads the offsets back inside the call: they too are produced behind the hold."""
    want = S.CASES["record_minhash"].truth()
    t, d, seq, qual, off = batch_inputs(21, quality=True, offsets=True)
    with nt.RecordMinHash(21, BYTES, ctx=rig.ctx, **S.RMH) as rmh:
        def call():
            rmh.run_device(seq.buf, t.n, off.buf, S.N_RECORDS, NORMALIZE, d_qual=qual.buf, quality_cutoff=CUTOFF)

        def check(_, __, got, what):
            S.assert_answer(dict(zip(("offsets", "n_windows", "hashes", "counts"), got)), want, what)
        run(rig, "record_minhash", SYNC, [seq, qual, off], [], call, check, read=rmh.sketches)
        # ntk_record_minhash_trim frees every array: with a hold pending it has to wait for the stream first, and the result is gone after it
        S.hazard_call(rig, SYNC, [], [], rmh.trim)
        assert rmh.stats()["n_entries"] == 0 and rmh.sketches()[2].size == 0


def test_kmer_colors_run_and_lookup(rig):
    """ntk_kmer_colors_run_device and ntk_kmer_colors_lookup_device against an index that is complete: each under a hold of its own."""
    want = S.CASES["colors_screen"].truth()
    t, d, seq, qual, off = batch_inputs(21, quality=True, offsets=True)
    q = S.color_queries()
    queries = S.words_input(q, q ^ np.uint64(1))
    rows = torch.zeros((S.N_RECORDS, 5), dtype=torch.int64, device="cuda")
    hits, single = torch.zeros((S.N_RECORDS, S.N_COLORS), dtype=torch.int64, device="cuda"), torch.zeros((S.N_RECORDS, S.N_COLORS), dtype=torch.int64, device="cuda")
    masks = torch.zeros(q.size, dtype=torch.int64, device="cuda")
    p = params(21, BYTES, NORMALIZE, CUTOFF)
    kt, st, mt = S.color_lists("true")
    with nt.KmerColors(21, BYTES, S.N_COLORS, CAPACITY, rig.ctx) as kc:
        kc.add_masks(np.concatenate([kt, st]), np.concatenate([np.ones(kt.size, dtype=np.uint64), mt]))

        def screen():
            kc._check("run_device", kc._h, ptr(seq.buf), ptr(qual.buf), t.n, ptr(off.buf), S.N_RECORDS, C.byref(p), ptr(rows), ptr(hits), ptr(single))

        def check_screen(_, clones, __, what):
            S.assert_answer(dict(zip(("rows", "hits", "single"), (S.host(c) for c in clones))), {key: want[key] for key in ("rows", "hits", "single")}, what)
        run(rig, "colors_screen", SYNC, [seq, qual, off], [rows, hits, single], screen, check_screen)

        def lookup():
            kc._check("lookup_device", kc._h, ptr(queries.buf), q.size, ptr(masks))
        run(rig, "colors_lookup", SYNC, [queries], [masks], lookup, lambda _, clones, __, what: S.assert_answer({"lookup": S.host(clones[0])}, {"lookup": want["lookup"]}, what))


def extract(table, min_count, keys, counts, cap):
    n = u64(0)
    table._check("extract_device", table._h, min_count, ptr(keys), ptr(counts), cap, C.byref(n))
    return int(n.value)


@pytest.mark.parametrize("words", list(S.KSETS))
def test_kmer_sets(rig, words):
    """ntk_kmer_sets_validate / compare / apply_device on the list ntk_kmer_table_extract_device (ntk_wide_table_extract_device) wrote
    in the same chain: the table is reset, counts and is extracted behind one hold; every set call is then made behind a hold of its own,
    with the extracted tensors copied into its inputs behind that hold."""
    import _kmer_sets_model as KS
    k = S.KSETS[words]
    ka, ca, kb, cb = S.kset_lists(words, "true")
    kd, cd, _, _ = S.kset_lists(words, "decoy")
    n, nb = int(ca.size), int(cb.size)
    full = S.CASES[f"count_table-{'narrow' if words == 1 else 'wide'}"].truth()
    want = S.CASES[f"kmer_sets-{words}"].truth()
    t, d, seq, _, _ = batch_inputs(k)
    cap = t.n
    x_keys, x_counts = torch.zeros(words * cap, dtype=torch.int64, device="cuda"), torch.zeros(cap, dtype=torch.int64, device="cuda")
    lib = ks_lib.lib()
    h = C.c_void_p()
    NL.check(lib.ntk_kmer_sets_create(rig.ctx._h, words, C.byref(h)), "ntk_kmer_sets_create")
    with (nt.KmerTable if words == 1 else nt.WideKmerTable)(k, BYTES, CAPACITY, rig.ctx) as table:
        try:
            def count_and_extract():
                table.reset()
                table.count_device(seq.buf, t.n, NORMALIZE)
                return extract(table, 1, x_keys, x_counts, cap)

            def check_extract(got_n, clones, __, what):
                assert got_n == full["n_distinct"], what
                S.assert_answer({"keys": S.host(clones[0])[:words * got_n].reshape(full["keys"].shape), "counts": S.host(clones[1])[:got_n]},
                                {"keys": full["keys"], "counts": full["counts"]}, what)
            run(rig, f"extract-{words}", SYNC, [seq], [x_keys, x_counts], count_and_extract, check_extract)
            # the device's own list goes on (cut to the length it shares with the decoy's): nothing of it came through the host
            keys = S.Input(x_keys[:words * n].clone(), S.dev_words(kd), 0)
            counts = S.Input(x_counts[:n].clone(), S.dev_words(cd), 0)
            torch.cuda.synchronize()
            b_keys, b_counts = S.dev_words(kb), S.dev_words(cb)

            flipped = S.Input(keys.true, S.dev_words(ka[::-1]), 0)

            def validate():
                v = u64(0)
                NL.check(lib.ntk_kmer_sets_validate_device(h, ptr(flipped.buf), n, C.byref(v)), "validate")
                return int(v.value)
            run(rig, f"kmer_sets_validate-{words}", SYNC, [flipped], [], validate,
                lambda v, _, __, what: S.assert_answer({"violations": v}, S.CASES[f"kmer_sets_validate-{words}"].truth(), what))

            def compare():
                hist, tot = np.zeros(S.KSET_BINS[0] * S.KSET_BINS[1], dtype=np.uint64), ks_lib.Totals()
                NL.check(lib.ntk_kmer_sets_compare_device(h, ptr(keys.buf), ptr(counts.buf), n, ptr(b_keys), ptr(b_counts), nb, S.KSET_BINS[0],
                                                          S.KSET_BINS[1], hist.ctypes.data, C.byref(tot)), "compare")
                return hist, tuple(int(getattr(tot, name)) for name in KS.TOTALS)
            run(rig, f"kmer_sets_compare-{words}", SYNC, [keys, counts], [], compare,
                lambda r, _, __, what: S.assert_answer({"hist": r[0], "totals": r[1]}, {"hist": want["hist"], "totals": want["totals"]}, what))

            for op, rule, name, bound in ((ks_lib.INTERSECT, ks_lib.MIN, "intersect", min(n, nb)), (ks_lib.UNION, ks_lib.SUM, "union", n + nb)):
                o_keys, o_counts = torch.zeros(words * bound, dtype=torch.int64, device="cuda"), torch.zeros(bound, dtype=torch.int64, device="cuda")

                def apply(op=op, rule=rule, o_keys=o_keys, o_counts=o_counts, bound=bound):
                    m = u64(0)
                    NL.check(lib.ntk_kmer_sets_apply_device(h, op, rule, ptr(keys.buf), ptr(counts.buf), n, ptr(b_keys), ptr(b_counts), nb,
                                                            ptr(o_keys), ptr(o_counts), bound, C.byref(m)), "apply")
                    return int(m.value)

                def check_apply(m, clones, __, what, name=name):
                    wk, wc = want[f"{name}_keys"], want[f"{name}_counts"]
                    assert m == wc.size, (what, m, wc.size)
                    S.assert_answer({"keys": S.host(clones[0])[:words * m].reshape(wk.shape), "counts": S.host(clones[1])[:m]}, {"keys": wk, "counts": wc}, what)
                run(rig, f"kmer_sets_{name}-{words}", SYNC, [keys, counts], [o_keys, o_counts], apply, check_apply)
        finally:
            lib.ntk_kmer_sets_destroy(h)


def test_dbg(rig):
    """ntk_dbg_adjacency / unitigs / spell_device at k = 21, each behind a hold of its own with its list (and, for spell, the rows the
    unitigs call wrote on the device) produced behind it; the spelled batch is counted by a fresh table straight from the device."""
    import _dbg_model as DM
    want = S.CASES["dbg"].truth()
    (kt, ct), (kd, cd) = S.dbg_lists("true"), S.dbg_lists("decoy")
    n = int(kt.size)
    keys, counts = S.words_input(kt, kd), S.words_input(ct, cd)
    edges = torch.zeros(n, dtype=torch.uint8, device="cuda")
    kmer_rows, unitig_rows = torch.zeros((n, 2), dtype=torch.int32, device="cuda"), torch.zeros((n, 4), dtype=torch.int64, device="cuda")
    cap_bytes = (n * 22 + 15) // 16 * 16
    seq_out, offsets_out = torch.zeros(cap_bytes + 64, dtype=torch.uint8, device="cuda"), torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    lib = dbg_lib.lib()
    h = C.c_void_p()
    NL.check(lib.ntk_dbg_create(rig.ctx._h, 21, C.byref(h)), "ntk_dbg_create")
    try:
        def adjacency():
            tot = dbg_lib.Totals()
            NL.check(lib.ntk_dbg_adjacency_device(h, ptr(keys.buf), n, ptr(edges), C.byref(tot)), "adjacency")
            return tuple(np.array([[int(v) for v in row] for row in tot.deg_hist], dtype=np.uint64).tolist() if name == "deg_hist" else int(getattr(tot, name))
                         for name in DM.TOTALS)
        run(rig, "dbg_adjacency", SYNC, [keys], [edges], adjacency,
            lambda tot, clones, __, what: S.assert_answer({"edges": S.host(clones[0]), "totals": tot}, {"edges": want["edges"], "totals": want["totals"]}, what))

        def unitigs():
            nu, nbases = u64(0), u64(0)
            NL.check(lib.ntk_dbg_unitigs_device(h, ptr(keys.buf), ptr(counts.buf), n, ptr(kmer_rows), ptr(unitig_rows), n, C.byref(nu), C.byref(nbases)), "unitigs")
            return int(nu.value), int(nbases.value)
        held = {}

        def check_unitigs(r, clones, __, what):
            nu, nbases = r
            assert (nu, nbases) == (want["n_unitigs"], want["n_bases"]), what
            S.assert_answer({"kmer_rows": clones[0].cpu().numpy().view(np.uint32), "unitig_rows": S.host(clones[1])[:nu]},
                            {"kmer_rows": want["kmer_rows"], "unitig_rows": want["unitig_rows"]}, what)
            held["rows"] = clones
        run(rig, "dbg_unitigs", SYNC, [keys, counts], [kmer_rows, unitig_rows], unitigs, check_unitigs)
        nu = want["n_unitigs"]
        in_kmer, in_unitig = S.Input(held["rows"][0], torch.zeros_like(held["rows"][0]), 0), S.Input(held["rows"][1], torch.zeros_like(held["rows"][1]), 0)
        with nt.KmerTable(21, BYTES, CAPACITY, rig.ctx) as fresh:
            def spell():
                nbytes, nrec = u64(0), u64(0)
                NL.check(lib.ntk_dbg_spell_device(h, ptr(keys.buf), n, ptr(in_kmer.buf), ptr(in_unitig.buf), nu, ptr(seq_out), cap_bytes, ptr(offsets_out),
                                                  nu, C.byref(nbytes), C.byref(nrec)), "spell")
                held["n_bytes"] = int(nbytes.value)
                return int(nbytes.value), int(nrec.value)

            def recount():
                fresh.reset()
                fresh.count_device(seq_out, held["n_bytes"], NORMALIZE)
                return fresh.items()

            def check_spell(r, clones, got, what):
                nbytes, nrec = r
                assert nrec == nu and nbytes == int(want["offsets"][-1]), what
                text = S.host(clones[0])
                S.assert_answer({"text": text[:want["text"].size], "offsets": S.host(clones[1])[:nu + 1], "recount_keys": got[0]},
                                {key: want[key] for key in ("text", "offsets", "recount_keys")}, what)
                assert bool((text[want["text"].size:(nbytes + 15) // 16 * 16] == ord("\n")).all()), what
                assert np.array_equal(got[1], np.ones(got[0].size, dtype=np.uint64)), what
            run(rig, "dbg_spell", SYNC, [keys, in_kmer, in_unitig], [seq_out, offsets_out], spell, check_spell, read=recount)
    finally:
        lib.ntk_dbg_destroy(h)


def test_mhset_compare(rig):
    """ntk_mhset_compare after ntk_mhset_add takes host inputs: with a hold pending, the result is right and the stream is drained at the
    return."""
    import _mhset_model as SM
    want = S.CASES["mhset_compare"].truth()
    sketches = S.mhset_sketches()
    with nt.MinHashSet(True, rig.ctx) as s:
        def call():
            s.reset()
            for hashes, counts in sketches:
                s.add((hashes, counts))
            return s.compare(num=64, max_hash=S.M64)

        def check(got, _, __, what):
            for name in SM.MATRICES + ("n_a", "n_b"):
                assert got[name].dtype == want[name].dtype and np.array_equal(got[name], want[name]), (what, name)
        run(rig, "mhset_compare", SYNC, [], [], call, check)
        got, _, _ = S.hazard_call(rig, SYNC, [], [], lambda: s.sketch(3))   # ntk_mhset_read, from the device copy
        assert np.array_equal(got[0], sketches[3][0]) and np.array_equal(got[1], sketches[3][1])


def test_merges_from_host_arrays(rig):
    """ntk_kmer_sketch_merge and ntk_minhash_merge take host arrays and synchronise: with the handle's own add_device queued behind a hold,
    the merge folds into all of it, and the stream is drained at the return."""
    import _minhash_model as MH
    import _sketch_model as SK
    want = S.CASES["host_merges"].truth()
    t, d, seq, _, _ = batch_inputs(21)
    d_keys = S.keys_answer(d.buf, 21, BYTES, NORMALIZE)
    regs, (hashes, counts) = SK.registers(d_keys), MH.sketch(d_keys, **S.MINHASH)
    ctx = rig.ctx
    with nt.KmerSketch(21, BYTES, ctx) as sk, nt.KmerMinHash(21, BYTES, ctx=ctx, **S.MINHASH) as mh:
        def sketch_merge():
            sk.reset()
            sk.add_device(seq.buf, t.n, NORMALIZE)
            sk.merge(regs, n_windows=int(d_keys.shape[0]))

        def minhash_merge():
            mh.reset()
            mh.add_device(seq.buf, t.n, NORMALIZE)
            mh.merge(hashes, counts, n_windows=int(d_keys.shape[0]))

        run(rig, "sketch_merge", SYNC, [seq], [], sketch_merge,
            lambda _, __, got, what: S.assert_answer(got, {"registers": want["registers"], "n_windows": want["sketch_n_windows"]}, what), read=lambda: read_sketch(sk))

        def read():
            (h, c), st = mh.hashes(), mh.stats()
            return {"hashes": h, "counts": c, "n_windows": st["n_windows"]}
        run(rig, "minhash_merge", SYNC, [seq], [], minhash_merge,
            lambda _, __, got, what: S.assert_answer(got, {"hashes": want["hashes"], "counts": want["counts"], "n_windows": want["minhash_n_windows"]}, what), read=read)


# ---- one chain like a user's ------------------------------------------------------------------------------------------------------------------

def test_a_chain_like_a_users(rig):
    """trim and compact -> a fresh table counts the kept reads -> its extract_device -> intersected with the reference's list -> unitigs,
    spelled -> per-record sketches of the unitig batch.  The batch is produced behind the first hold; after that every stage takes the
    device tensors the stage before wrote, with nothing of ours between them but a hold and the poison of its own outputs, and every
    stage is compared with its model."""
    import _dbg_model as DM  # noqa: F401
    want = S.CASES["chain"].truth()
    t, d, seq, qual, off = batch_inputs(21, quality=True, offsets=True)
    ref = S.items_answer(b"".join(r + b"\n" for r in t.records[::2] + d.records[1::2]), 21, BYTES, NORMALIZE)
    r_keys, r_counts = S.dev_words(ref[0]), S.dev_words(ref[1])
    b = TrimBuffers(t.n, S.N_RECORDS)
    p = params(21, BYTES, NORMALIZE, CUTOFF)
    cap = t.n
    x_keys, x_counts = torch.zeros(cap, dtype=torch.int64, device="cuda"), torch.zeros(cap, dtype=torch.int64, device="cuda")
    j_keys, j_counts = torch.zeros(cap, dtype=torch.int64, device="cuda"), torch.zeros(cap, dtype=torch.int64, device="cuda")
    kmer_rows, unitig_rows = torch.zeros((cap, 2), dtype=torch.int32, device="cuda"), torch.zeros((cap, 4), dtype=torch.int64, device="cuda")
    cap_bytes = (cap * 22 + 15) // 16 * 16
    u_seq, u_off = torch.zeros(cap_bytes + 64, dtype=torch.uint8, device="cuda"), torch.zeros(cap + 1, dtype=torch.int64, device="cuda")
    ks, dl = ks_lib.lib(), dbg_lib.lib()
    hs, hd = C.c_void_p(), C.c_void_p()
    NL.check(ks.ntk_kmer_sets_create(rig.ctx._h, 1, C.byref(hs)), "ntk_kmer_sets_create")
    NL.check(dl.ntk_dbg_create(rig.ctx._h, 21, C.byref(hd)), "ntk_dbg_create")
    n = {}
    with nt.KmerTable(21, BYTES, CAPACITY, rig.ctx) as table, nt.ReadTrimmer(table) as rt, nt.KmerTable(21, BYTES, CAPACITY, rig.ctx) as fresh, \
            nt.RecordMinHash(21, BYTES, ctx=rig.ctx, **S.CHAIN_RMH) as rmh:
        def trim():
            table.reset()
            table.count_device(seq.buf, t.n, NORMALIZE)
            n["kept_bytes"], n["kept"] = trim_and_compact(rt, p, seq.buf, qual.buf, t.n, off.buf, b)

        def count_and_extract():
            fresh.reset()
            fresh.count_device(b.seq, n["kept_bytes"], NORMALIZE)
            n["keys"] = extract(fresh, 1, x_keys, x_counts, cap)

        def intersect():
            m = u64(0)
            NL.check(ks.ntk_kmer_sets_apply_device(hs, ks_lib.INTERSECT, ks_lib.LEFT, ptr(x_keys), ptr(x_counts), n["keys"], ptr(r_keys), ptr(r_counts),
                                                   int(ref[1].size), ptr(j_keys), ptr(j_counts), min(n["keys"], int(ref[1].size)), C.byref(m)), "apply")
            n["joined"] = int(m.value)

        def unitigs():
            nu, nbases = u64(0), u64(0)
            NL.check(dl.ntk_dbg_unitigs_device(hd, ptr(j_keys), ptr(j_counts), n["joined"], ptr(kmer_rows), ptr(unitig_rows), n["joined"], C.byref(nu),
                                               C.byref(nbases)), "unitigs")
            n["unitigs"] = int(nu.value)

        def spell():
            nbytes, nrec = u64(0), u64(0)
            NL.check(dl.ntk_dbg_spell_device(hd, ptr(j_keys), n["joined"], ptr(kmer_rows), ptr(unitig_rows), n["unitigs"], ptr(u_seq), cap_bytes, ptr(u_off),
                                             n["unitigs"], C.byref(nbytes), C.byref(nrec)), "spell")
            n["unitig_bytes"] = int(nbytes.value)

        def sketch():
            rmh.run_device(u_seq, n["unitig_bytes"], u_off, n["unitigs"], NORMALIZE)

        stages = ((trim, [seq, qual, off], b.all(), None), (count_and_extract, [], [x_keys, x_counts], None), (intersect, [], [j_keys, j_counts], None),
                  (unitigs, [], [kmer_rows, unitig_rows], None), (spell, [], [u_seq, u_off], None), (sketch, [], [], rmh.sketches))
        try:
            for plain in (True, False):
                what = "warm-up" if plain else "hazard"
                got = {}
                for stage, inputs, outputs, read in stages:
                    # (the inputs of the first stage are not clobbered: the later stages read nothing of them, but the chain is one pass)
                    _, clones, r = S.hazard_call(rig, SYNC, inputs, outputs, stage, read, plain=plain)
                    got[stage.__name__] = (clones, r)
                rows, kept = S.host(got["trim"][0][0]), S.host(got["trim"][0][1])[:n["kept_bytes"]]
                sk = got["sketch"][1]
                S.assert_answer({"trim_rows": rows, "kept": kept, "table_keys": S.host(got["count_and_extract"][0][0])[:n["keys"]],
                                 "table_counts": S.host(got["count_and_extract"][0][1])[:n["keys"]], "joined_keys": S.host(got["intersect"][0][0])[:n["joined"]],
                                 "joined_counts": S.host(got["intersect"][0][1])[:n["joined"]], "unitig_rows": S.host(got["unitigs"][0][1])[:n["unitigs"]],
                                 "unitig_text": S.host(got["spell"][0][0])[:want["unitig_text"].size], "sketch_offsets": sk[0], "sketch_hashes": sk[2],
                                 "sketch_counts": sk[3]}, want, what)
        finally:
            ks.ntk_kmer_sets_destroy(hs)
            dl.ntk_dbg_destroy(hd)


# ---- the harness bites ----------------------------------------------------------------------------------------------------------------------

def test_negative_control_reads_the_decoy(rig):
    """A stand-in for a wrong call - the sum of the input queued on another stream with no event - run through the same hazard: it must
    return the decoy's sum (the copy of the true input sits behind the hold), and the true sum the plain way."""
    true, decoy = S.CASES["negative_control"].truth()["sum"], S.CASES["negative_control"].others()["decoy"]["sum"]
    t, d, seq, _, _ = batch_inputs(21)
    pad = (seq.buf.numel() - t.n) * ord("\n")
    got, _, _ = S.hazard_call(rig, ASYNC, [seq], [], lambda: S.wrong_stream_sum(rig, seq.buf), plain=True)
    assert got - pad == true
    got, _, _ = S.hazard_call(rig, ASYNC, [seq], [], lambda: S.wrong_stream_sum(rig, seq.buf))
    assert got - pad == decoy and decoy != true, (got - pad, decoy, true)
