"""The harness that holds the device-face calls to their stream contract (tests/_stream_contract.py) while the context's stream is busy:
shared by tests/test_gpu_stream_order.py (the cases on a real MI355X) and tests/test_stream_order_inputs.py (CPU: the cases are not
vacuous).  Importable without a GPU: torch is imported only inside the device functions.

The idea.  Every other GPU test hands a call an input that is complete and reads its result after a device-wide synchronisation, so the
host is what orders the caller's producer, the library's kernels and the caller's consumer.  Here the stream orders them.  `hazard_call`
queues, on the stream the context works on and with no host wait in between: a bounded spin (`Rig.hold`), the copies that turn the DECOY
every input buffer holds into the TRUE input, a poison fill of every output, the call itself, a CLOBBER of every input (write after
read), and clones of the outputs (the consumer).  A kernel, a memset or a rocPRIM call queued on another stream, a host decision taken
from device data the stream has not produced yet, a "synchronous" call that returns with work queued, or an output written ahead of the
caller's own write to that buffer then reads the decoy, loses its result to the poison, or sees the clobber - and every one of those
gives another answer than the true input (tests/test_stream_order_inputs.py proves that per case from the host models alone).

The decoy of a batch has the same byte length, other bases and no N; the decoy of an offsets array is all zero (every record empty: valid
under the headers, "An offset beyond n_bytes is read as n_bytes"); the clobber of a batch is an all-'N' fill, of a quality stream and of a
list of words an all-zero fill.  Truth is the host models the suite already has; every comparison is exact.

The negative control (`wrong_stream_sum`) is a torch-only stand-in for a call that queues its work on another stream without an event:
run through `hazard_call` it reads the decoy.  No kernel and no library is altered for it (tools/mutation_audit.py states the rule)."""
import ctypes as C
import math
import time

import numpy as np

import needletail_amd as nt
import oracle as O
from needletail_amd import _lib as NL

ASYNC, MAY_SYNC, SYNC = "ASYNC", "MAY_SYNC", "SYNC"
SEED = 0x57E4D                      # the one seed of every input here
POISON = 0x5A                       # the byte every output holds when the call is made ('Z': no base, not a break byte of the packer)
POISON_WORD = 0x5A5A5A5A5A5A5A5A
CUTOFF = 53
MIN_HOLD_MS, MAX_SPIN_MS = 20.0, 200.0
N_RECORDS = 48
BYTES, BITS, BITS_CANON = nt.PATH_BYTES_CANONICAL, nt.PATH_BITS, nt.PATH_BITS_CANONICAL
NONE, NORMALIZE = nt.PRE_NONE, nt.PRE_NORMALIZE
M64 = (1 << 64) - 1
_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_COMP = {65: 84, 67: 71, 71: 67, 84: 65}


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------

def record_lengths(k: int):
    """48 record lengths from {0, 1, k - 1, k, 150, 700}, about 6 KB, in a fixed shuffled order."""
    lens = [0] * 5 + [1] * 5 + [k - 1] * 5 + [k] * 7 + [150] * 22 + [700] * 4
    assert len(lens) == N_RECORDS
    return [lens[i] for i in np.random.default_rng([SEED, 1, k]).permutation(N_RECORDS)]


class Batch:
    """records (bytes each), quals (uint8 arrays) and their packed forms: buf (one '\\n' after every record), qual (a byte per byte of
    buf; 0xFF under the break bytes) and offsets (uint64, n_records + 1)."""

    def __init__(self, records, quals):
        self.records, self.quals = list(records), list(quals)
        self.buf = b"".join(r + b"\n" for r in self.records)
        self.qual = np.concatenate([np.append(q, np.uint8(0xFF)) for q in self.quals]).astype(np.uint8)
        self.offsets = np.concatenate([[0], np.cumsum([len(r) + 1 for r in self.records])]).astype(np.uint64)
        assert self.qual.size == len(self.buf) == int(self.offsets[-1])

    @property
    def n(self) -> int:
        return len(self.buf)


def _qualities(rng, L, masked_share):
    q = np.full(L, 70, dtype=np.uint8)
    q[rng.random(L) < masked_share] = CUTOFF - 1
    return q


def true_batch(k: int, lower: bool = False, repeat: bool = False) -> Batch:
    """The true input of a case at k: random bases, a run of N in every 700-base record and in every fourth 150-base one, 5 % of the
    quality bytes below CUTOFF, the last 150-base record an exact duplicate of the first.  lower: one lower-case base (the raw-byte routes redo the launch for it).  repeat: one inverted repeat
    of 2 (k + 8) bases in a 700-base record (a k-mer that ties with its reverse complement over 32 bases exists in it for even k and for
    k >= 65 only; tests/test_gpu_parity.py states the rule)."""
    rng = np.random.default_rng([SEED, 2, k])
    recs, quals, n150, did_lower, did_repeat, first150 = [], [], 0, False, False, None
    for L in record_lengths(k):
        a = _ACGT[rng.integers(0, 4, L)].copy()
        if L == 700:
            a[300:305] = ord("N")
            if repeat and not did_repeat:
                half = _ACGT[rng.integers(0, 4, k + 8)]
                a[20:20 + 2 * (k + 8)] = np.concatenate([half, np.array([_COMP[int(c)] for c in half[::-1]], dtype=np.uint8)])
                did_repeat = True
        if L == 150:
            n150 += 1
            if n150 == 1:
                first150 = a.copy()
            if n150 == 22:
                a = first150.copy()   # an exact duplicate of the first 150-base read: k-mers with count 2
            elif n150 % 4 == 0:
                a[70:73] = ord("N")
            elif lower and n150 == 2:
                a[75] |= 0x20
                did_lower = True
        recs.append(a.tobytes())
        quals.append(_qualities(rng, L, 0.05))
    assert did_lower == lower and did_repeat == repeat
    return Batch(recs, quals)


def decoy_batch(k: int) -> Batch:
    """Valid input of the same record lengths (so the same byte length and break bytes) with other bases, no N, no lower case, and a
    quality stream that masks a fifth of the bases."""
    rng = np.random.default_rng([SEED, 3, k])
    lens = record_lengths(k)
    return Batch([_ACGT[rng.integers(0, 4, L)].tobytes() for L in lens], [_qualities(rng, L, 0.2) for L in lens])


def clobber_bytes(n: int) -> bytes:
    return b"N" * n


def records_of(buf: bytes, offsets) -> list:
    """The records a call sees in buf under `offsets`: [offsets[r], offsets[r + 1]) without its last byte, the break byte; nothing where
    the range is empty (the all-zero decoy offsets)."""
    off = [min(int(o), len(buf)) for o in offsets]
    return [buf[off[r]:max(off[r + 1] - 1, off[r])] for r in range(len(off) - 1)]


def quals_of(qual: np.ndarray, offsets) -> list:
    off = [min(int(o), qual.size) for o in offsets]
    return [qual[off[r]:max(off[r + 1] - 1, off[r])] for r in range(len(off) - 1)]


def stride_records(seed_tag: int, n_records: int = N_RECORDS, record_len: int = 100) -> bytes:
    """Fixed-stride records (record_len bases and a '\\n') for ntk_reverse_complement_records_device."""
    rng = np.random.default_rng([SEED, 4, seed_tag])
    return b"".join(_ACGT[rng.integers(0, 4, record_len)].tobytes() + b"\n" for _ in range(n_records))


# ---- truth: the suite's host models ---------------------------------------------------------------------------------------------------------

STATS_KEYS = ("n_total", "n_fwd", "n_rc", "sum", "xor", "hist")
WIDE_KEYS = ("n_total", "n_fwd", "n_rc", "hist")      # k > 32: a 2-bit value of more than 64 bits has no sum / xor


def masked(buf: bytes, qual, cutoff: int = CUTOFF) -> bytes:
    """QualitySequence::quality_mask over a packed batch (qual None: no mask)."""
    return buf if qual is None else O.quality_mask(buf, np.asarray(qual, dtype=np.uint8).tobytes(), cutoff)


def reduce_answer(buf: bytes, k: int, path: int, pre: int, qual=None) -> dict:
    """What ntk_reduce_device(_quality) accumulates from an empty result: the oracle's record chain for k <= 32, the literal wide
    iterator of tests/test_gpu_lower_watch.py for k = 33..255."""
    text = masked(buf, qual)
    if k <= 32:
        st = O.reduce_records(text.split(b"\n"), k, path, pre)
        return {key: st[key] for key in STATS_KEYS}
    from test_gpu_lower_watch import _wide_reference   # (its module imports torch)
    st = _wide_reference(text.split(b"\n"), k, pre >= NORMALIZE)
    return {key: st[key] for key in WIDE_KEYS}


def minimizers_answer(buf: bytes, k: int, w: int) -> dict:
    st = O.minimizers_reduce(buf, k, w, True, True)
    return {key: st[key] for key in STATS_KEYS}


def add_stats(a: dict, b: dict) -> dict:
    out = {}
    for key in a:
        if key == "xor":
            out[key] = a[key] ^ b[key]
        elif key == "hist":
            out[key] = a[key] + b[key]
        else:
            out[key] = (a[key] + b[key]) & M64
    return out


def planes_answer(buf: bytes, k: int, path: int, pre: int, qual=None) -> dict:
    """The three planes of ntk_materialize_device(_quality) per byte: valid, strand where valid, value where valid."""
    from test_gpu_build_matrix import expected_planes   # (its module imports torch)
    valid, rcf, vals = expected_planes(masked(buf, qual), k, path, pre)
    return {"valid": valid, "rc": rcf & valid, "values": np.where(valid, vals, np.uint64(0))}


def rc_records_answer(buf: bytes, n_records: int, record_len: int, stride: int) -> np.ndarray:
    out = bytearray(buf)
    for r in range(n_records):
        out[r * stride:r * stride + record_len] = O.reverse_complement(buf[r * stride:r * stride + record_len])
    return np.frombuffer(bytes(out), dtype=np.uint8)


def items_answer(buf: bytes, k: int, path: int, pre: int, qual=None):
    """(keys, counts) of a count table that counted the batch from empty: narrow values, or [hi, lo] rows at k >= 33."""
    import _lib_fuzz as F
    keys, counts = F.items_of(masked(buf, qual), k, path, pre)
    return keys, counts.astype(np.uint64)


def keys_answer(buf: bytes, k: int, path: int, pre: int, qual=None) -> np.ndarray:
    """Every key the batch emits, with repeats."""
    import _lib_fuzz as F
    return F.oracle_keys(masked(buf, qual), k, path, pre)


def differs(a, b) -> bool:
    """Two answers of one kind differ: as arrays, or as numbers."""
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.asarray(a), np.asarray(b)
        return a.shape != b.shape or not np.array_equal(a, b)
    return a != b


def assert_answers_differ(true: dict, other: dict, what):
    """Every field and array the GPU test compares tells the two inputs apart."""
    assert set(true) == set(other), what
    for key in true:
        assert differs(true[key], other[key]), (what, key)


def assert_answer(got: dict, want: dict, what):
    for key in want:
        assert not differs(got[key], want[key]), (what, key, got[key], want[key])


# ---- the device side ------------------------------------------------------------------------------------------------------------------------

_CAL = {}


def cycles_per_ms() -> float:
    """torch.cuda._sleep cycles per millisecond of this device's clock, measured once per session with two events on an otherwise idle
    stream: from 10^5 cycles, times 8 until one spin measures at least 1 ms."""
    import torch
    if "cpm" not in _CAL:
        s = torch.cuda.Stream()
        cycles, tries = 10 ** 5, []
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)   # (the first launch of the spin kernel loads it)
            s.synchronize()
            while True:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                torch.cuda._sleep(cycles)
                e1.record(s)
                s.synchronize()
                ms = e0.elapsed_time(e1)
                tries.append((cycles, ms))
                if ms >= 1.0:
                    break
                cycles *= 8
                assert cycles < 10 ** 13, tries
        _CAL["cpm"], _CAL["calibration"] = cycles / ms, tries
        print(f"stream_order: calibration {tries}: {_CAL['cpm']:.0f} cycles per ms")
    return _CAL["cpm"]


def set_hold_ms(return_times_ms: dict) -> float:
    """The hold of the session: the larger of 20 ms and ten times the longest host-side return time of an ASYNC call."""
    longest = max(return_times_ms.values()) if return_times_ms else 0.0
    _CAL["hold_ms"], _CAL["returns"] = max(MIN_HOLD_MS, 10.0 * longest), dict(return_times_ms)
    return _CAL["hold_ms"]


def hold_ms() -> float:
    return _CAL.get("hold_ms", MIN_HOLD_MS)


class Rig:
    """A non-blocking side stream and a context that works on it.  own_stream: the context owns its stream (nt.Context(0)), which is
    wrapped for torch with ExternalStream from the pointer ntk_ctx_stream gives."""

    def __init__(self, own_stream: bool = False):
        import torch
        if own_stream:
            self.ctx = nt.Context(0)
            dev, ptr = C.c_int(-1), C.c_void_p()
            NL.check(NL.lib().ntk_ctx_stream(self.ctx._h, C.byref(dev), C.byref(ptr)), "ntk_ctx_stream")
            assert dev.value == 0 and ptr.value, "a context that owns its stream has a stream of its own"
            self.side = torch.cuda.ExternalStream(ptr.value)
        else:
            self.side = torch.cuda.Stream()
            self.ctx = nt.Context(0, stream=self.side.cuda_stream)
        self.queued_ms = 0.0

    def close(self):
        self.side.synchronize()
        self.ctx.close()

    def hold(self, ms: float = None):
        """Queue a bounded spin of `ms` (default: the session's hold) on the side stream, in spins of at most 200 ms each."""
        import torch
        ms = hold_ms() if ms is None else ms
        pieces = max(1, math.ceil(ms / MAX_SPIN_MS))
        cycles = int(ms / pieces * cycles_per_ms())
        assert cycles / cycles_per_ms() <= MAX_SPIN_MS
        with torch.cuda.stream(self.side):
            for _ in range(pieces):
                torch.cuda._sleep(cycles)
        self.queued_ms += ms


def dev_bytes(data: bytes, fill: int = ord("\n")):
    """A device batch buffer: the bytes, then `fill` up to the next multiple of 16 and 64 more; complete when this returns."""
    import torch
    n = len(data)
    t = torch.full(((n + 15) // 16 * 16 + 64,), fill, dtype=torch.uint8, device="cuda")
    if n:
        t[:n] = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return t


def dev_words(a):
    """uint64 words as a device int64 tensor (at least one word); complete when this returns."""
    import torch
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    t = torch.zeros(max(a.size, 1), dtype=torch.int64, device="cuda")
    if a.size:
        t[:a.size] = torch.from_numpy(a.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    return t


def host(t) -> np.ndarray:
    a = t.cpu().numpy()
    return a.view(np.uint64) if a.dtype == np.int64 else a


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Input:
    """One input buffer of a call: `buf` is what the call is given; it holds `decoy` when the hazard run starts, `true` is copied over
    it behind the hold, and `clobber` (a fill value) is written over it behind the call."""

    def __init__(self, true, decoy, clobber: int):
        assert true.shape == decoy.shape and true.dtype == decoy.dtype
        self.true, self.decoy, self.clobber = true, decoy, clobber
        self.buf = decoy.clone()


def batch_input(true: bytes, decoy: bytes, clobber: int = ord("N")) -> Input:
    assert len(true) == len(decoy)
    return Input(dev_bytes(true), dev_bytes(decoy), clobber)


def words_input(true, decoy, clobber: int = 0) -> Input:
    return Input(dev_words(true), dev_words(decoy), clobber)


def hazard_call(rig: Rig, kind: str, inputs, outputs, call, read=None, plain: bool = False, clobber: bool = True):
    """One call under the hazard (module docstring), or - plain - the same call the ordinary way, which is every handle's warm-up.
    inputs: Input objects; outputs: device tensors the call writes; call(): makes the library call(s) on rig.ctx and returns what the
    host got back; read(): the reading calls of the library's header, made after the clobber is queued and before any host wait of
    ours.  Returns (what call returned, the clones of the outputs, what read returned).  Asserts the case's own preconditions: the
    producer is pending when the call is made; for ASYNC it is still pending when the call returns; for SYNC the stream is drained when
    the call returns."""
    import torch
    side = rig.side
    assert kind in (ASYNC, MAY_SYNC, SYNC)
    with torch.cuda.stream(side):
        for i in inputs:   # 1, 2: the decoy in every input, nothing in the outputs
            i.buf.copy_(i.true if plain else i.decoy)
        for out in outputs:
            out.zero_()
        side.synchronize()
        if not plain:
            rig.hold()                                   # 3
            for i in inputs:                             # 4: the producer
                i.buf.copy_(i.true, non_blocking=True)
        for out in outputs:                              # 5
            out.fill_(POISON if out.dtype == torch.uint8 else POISON_WORD if out.dtype == torch.int64 else 0x5A5A5A5A if out.dtype == torch.int32 else 0x5A5A)
        ev_in = torch.cuda.Event()
        ev_in.record(side)                               # 6
        rig.ev_in = ev_in                                # (a call of several parts asks it between them)
        if not plain:
            assert not ev_in.query(), "vacuous: the producer had finished before the call was made (the hold is too short)"
        result = call()                                  # 7
        if not plain and kind == ASYNC:                  # 8
            assert not ev_in.query(), "a call documented as asynchronous returned after its input was produced: it waited for the stream"
        if kind == SYNC:                                 # 11: the stream's own query, made before anything else is queued (an event recorded
            # here is itself work on the stream and takes microseconds to retire: its query right after the record says "not yet" on an idle stream)
            assert side.query(), "a call documented as synchronous returned with work still queued on the stream"
        if clobber:
            for i in inputs:                             # 9: the write after read
                i.buf.fill_(i.clobber)
        clones = [out.clone() for out in outputs]        # 10: the consumer, on the stream
        got = read() if read is not None else None
        side.synchronize()                               # 12
    return result, clones, got


def warm_then_hazard(rig: Rig, kind: str, inputs, outputs, call, check, read=None, clobber: bool = True):
    """The same call twice on the same handles and buffers: the plain way (the warm-up: every allocation happens here), then under the
    hazard; `check(result, clones, read result, what)` holds both to the model.  The call resets its handles itself, on the stream."""
    for plain in (True, False):
        result, clones, got = hazard_call(rig, kind, inputs, outputs, call, read, plain=plain, clobber=clobber)
        check(result, clones, got, "warm-up" if plain else "hazard")


def timed(rig: Rig, fn) -> float:
    """Host-side return time of fn() in ms on an idle stream (the handle is warm: fn ran before)."""
    rig.side.synchronize()
    t0 = time.perf_counter()
    fn()
    dt = (time.perf_counter() - t0) * 1e3
    rig.side.synchronize()
    return dt


def wrong_stream_sum(rig: Rig, t):
    """The stand-in for a wrong call: the sum of `t` queued on a second non-blocking stream with no event from the side stream.  It
    reads memory nothing is writing at that moment (the producer's copy sits behind the hold)."""
    import torch
    other = torch.cuda.Stream()
    with torch.cuda.stream(other):
        s = int(t.sum(dtype=torch.int64).item())   # (the copy back is queued on `other` too)
    return s


# ---- the cases: inputs and truth of every GPU test, in one place for the CPU test that proves them non-vacuous ------------------------------

class Case:
    """truth(): the answer for the true input, a dict of the fields and arrays the GPU test compares.  others(): name -> the answer the
    same comparison would see if the call had read the decoy, seen the clobber, or lost or misplaced a stage of its chain; every one
    must differ from the truth in every field."""

    def __init__(self, name, truth, others):
        self.name, self._truth, self._others, self._cache = name, truth, others, {}

    def truth(self) -> dict:
        if "truth" not in self._cache:
            self._cache["truth"] = self._truth()
        return self._cache["truth"]

    def others(self) -> dict:
        return {name: fn() for name, fn in self._others.items()}


CASES = {}
_BATCHES = {}


def batches(k: int, lower: bool = False, repeat: bool = False):
    """(true, decoy) of a case at k, made once."""
    key = (k, lower, repeat)
    if key not in _BATCHES:
        _BATCHES[key] = (true_batch(k, lower, repeat), decoy_batch(k))
        assert _BATCHES[key][0].n == _BATCHES[key][1].n and 5000 <= _BATCHES[key][0].n <= 8000
    return _BATCHES[key]


def _case(name, truth, **others):
    assert name not in CASES, name
    CASES[name] = Case(name, truth, others)
    return CASES[name]


def _zero_qual(n):
    return np.zeros(n, dtype=np.uint8)


# (k, path, pre, lower, repeat) of the four reduce routes
REDUCE_ROUTES = {
    "k21_bytes_normalize": (21, BYTES, NORMALIZE, False, False),   # scan2, the packed-value build
    "k31_bits_none": (31, BITS_CANON, NONE, False, False),
    "k21_raw_lower": (21, BYTES, NONE, True, False),               # the speculative pair, the redo taken
    "k47_raw_lower": (47, BYTES, NONE, True, True),                # the packed-stream kernel and its byte-walking redo
}
REDUCE_IDS = [f"{route}-{'quality' if q else 'plain'}" for route in REDUCE_ROUTES for q in (False, True)]


def _reduce_cases():
    for route, (k, path, pre, lower, repeat) in REDUCE_ROUTES.items():
        for quality in (False, True):
            def truth(k=k, path=path, pre=pre, lower=lower, repeat=repeat, quality=quality):
                t, _ = batches(k, lower, repeat)
                return reduce_answer(t.buf, k, path, pre, t.qual if quality else None)

            def decoy(k=k, path=path, pre=pre, lower=lower, repeat=repeat, quality=quality):
                _, d = batches(k, lower, repeat)
                return reduce_answer(d.buf, k, path, pre, d.qual if quality else None)

            def clob(k=k, path=path, pre=pre, lower=lower, repeat=repeat, quality=quality):
                t, _ = batches(k, lower, repeat)
                return reduce_answer(clobber_bytes(t.n), k, path, pre, _zero_qual(t.n) if quality else None)

            others = dict(decoy=decoy, clobber=clob)
            if quality:   # the quality stream alone clobbered (all masked), and alone the decoy's
                others["quality_clobber"] = lambda k=k, path=path, pre=pre, lower=lower, repeat=repeat: reduce_answer(
                    batches(k, lower, repeat)[0].buf, k, path, pre, _zero_qual(batches(k, lower, repeat)[0].n))
                others["quality_decoy"] = lambda k=k, path=path, pre=pre, lower=lower, repeat=repeat: reduce_answer(
                    batches(k, lower, repeat)[0].buf, k, path, pre, batches(k, lower, repeat)[1].qual)
            _case(f"reduce-{route}-{'quality' if quality else 'plain'}", truth, **others)


_reduce_cases()


def _k21(which: str):
    t, d = batches(21)
    return {"true": t, "decoy": d}[which]


def _r21(buf, qual=None):
    return reduce_answer(buf, 21, BYTES, NORMALIZE, qual)


# a reduce of the decoy is queued ahead; the zeroing (NTK_FLAG_RESET folded into the launch, or ntk_accum_reset) must land between the two
for _name in ("reset_flag", "accum_reset"):
    _case(_name, lambda: _r21(_k21("true").buf),
          decoy=lambda: _r21(_k21("decoy").buf), clobber=lambda: _r21(clobber_bytes(_k21("true").n)),
          zeroing_ahead_of_both_or_lost=lambda: add_stats(_r21(_k21("decoy").buf), _r21(_k21("true").buf)))
_case("accum_bind", lambda: _r21(_k21("true").buf), decoy=lambda: _r21(_k21("decoy").buf), clobber=lambda: _r21(clobber_bytes(_k21("true").n)))
_case("own_stream", lambda: _r21(_k21("true").buf), decoy=lambda: _r21(_k21("decoy").buf), clobber=lambda: _r21(clobber_bytes(_k21("true").n)))
_case("batch_submit", lambda: _r21(_k21("true").buf), scan_ahead_of_the_reset=lambda: {key: (np.zeros(4096, np.uint64) if key == "hist" else 0) for key in STATS_KEYS},
      reset_lost=lambda: add_stats(_r21(_k21("decoy").buf), _r21(_k21("true").buf)))

# (k, w, NTK_OPT_MINIMIZER_ROUTE value): the register-fused build, the generic fused kernel, materialise + window-min
MINIMIZER_ROUTES = {"fused_21_11": (21, 11, 0), "generic_27_7": (27, 7, 0), "two_pass_21_11": (21, 11, NL.ROUTE_TWO_PASS)}
for _name, (_k, _w, _) in MINIMIZER_ROUTES.items():
    _case(f"minimizers-{_name}", lambda k=_k, w=_w: minimizers_answer(batches(k)[0].buf, k, w),
          decoy=lambda k=_k, w=_w: minimizers_answer(batches(k)[1].buf, k, w),
          clobber=lambda k=_k, w=_w: minimizers_answer(clobber_bytes(batches(k)[0].n), k, w))

MATERIALIZE_ROUTES = {"k21_bytes": (21, BYTES, NORMALIZE), "k31_bits": (31, BITS_CANON, NONE)}
MATERIALIZE_IDS = [f"{route}-{'quality' if q else 'plain'}" for route in MATERIALIZE_ROUTES for q in (False, True)]
for _route, (_k, _path, _pre) in MATERIALIZE_ROUTES.items():
    for _q in (False, True):
        _case(f"materialize-{_route}-{'quality' if _q else 'plain'}",
              lambda k=_k, p=_path, e=_pre, q=_q: planes_answer(batches(k)[0].buf, k, p, e, batches(k)[0].qual if q else None),
              decoy=lambda k=_k, p=_path, e=_pre, q=_q: planes_answer(batches(k)[1].buf, k, p, e, batches(k)[1].qual if q else None),
              clobber=lambda k=_k, p=_path, e=_pre, q=_q: planes_answer(clobber_bytes(batches(k)[0].n), k, p, e, _zero_qual(batches(k)[0].n) if q else None))

RC_RECORDS = (N_RECORDS, 100, 101)   # n_records, record_len, stride
_case("rc_records", lambda: {"out": rc_records_answer(stride_records(0), *RC_RECORDS)},
      decoy=lambda: {"out": rc_records_answer(stride_records(1), *RC_RECORDS)},
      clobber=lambda: {"out": rc_records_answer(clobber_bytes(len(stride_records(0))), *RC_RECORDS)})

SYNTH = (0x5EED57, 7, 40, 150, 6)   # seed, first_read, n_reads, read_len, n_per_1024
_case("synth_into_reduce", lambda: _r21(O.synth_reads(*SYNTH).tobytes()),
      synth_skipped=lambda: _r21(bytes([POISON]) * (SYNTH[2] * (SYNTH[3] + 1))))

# two reduces behind one hold.  The first batch (about 6 KB) is at most 8 tiles of the k = 21 build (stride 1004 bytes, ntk_tile.hpp
# sv2_stride_bytes), which one block of 12 waves pulls: plan_launch (ntk_plan.hpp) gives want_blocks = ceil(tiles / (chunk * waves)) = 1, so
# ensure_partials holds one row.  GROW_READS reads of 150 bases are 604 000 bytes = 602 tiles: chunk stays 1 (tiles < blocks_max * waves * 4
# on any device of 13 CUs or more) and want_blocks = ceil(602 / 12) = 51 rows (fewer only where the resident grid is smaller, and never 1),
# so d_part_hist must be replaced while the first reduce is queued.
GROW_READS = (0x5EED58, 0, 4000, 150, 6)
_case("two_reduces_partials_grow", lambda: add_stats(_r21(_k21("true").buf), _r21(O.synth_reads(*GROW_READS).tobytes())),
      first_lost=lambda: _r21(O.synth_reads(*GROW_READS).tobytes()), second_lost=lambda: _r21(_k21("true").buf),
      decoy=lambda: add_stats(_r21(_k21("decoy").buf), _r21(O.synth_reads(*GROW_READS).tobytes())))


# ---- the libraries ------------------------------------------------------------------------------------------------------------------------

TABLES = {"narrow": (21, BYTES, NORMALIZE), "wide": (47, BYTES, NORMALIZE)}


def table_queries(k, path, pre) -> np.ndarray:
    """What the table cases look up: every third key of the true batch and every seventh of the decoy's (canonical values, or [hi, lo] rows)."""
    t, d = batches(k)
    parts = [items_answer(t.buf, k, path, pre)[0][::3], items_answer(d.buf, k, path, pre)[0][::7]]
    if k == 21:   # and every eleventh of the larger batch of the growth case
        parts.append(items_answer(O.synth_reads(*GROW_COUNT_READS).tobytes(), k, path, pre)[0][::11])
    return np.concatenate(parts)


def _table_answer(k, path, pre, buf):
    import _lib_fuzz as F
    keys, counts = items_answer(buf, k, path, pre)
    spectrum = np.bincount(np.minimum(counts, 63).astype(np.int64), minlength=64).astype(np.uint64)
    return {"keys": keys, "counts": counts, "n_distinct": int(counts.size), "n_total": int(counts.sum()), "spectrum": spectrum,
            "lookup": F._lookup(table_queries(k, path, pre), (keys, counts))}


def _both(k, path, pre, fn):
    """What a table, sketch or index holds that also kept the decoy batch it was pre-loaded with: the reset ran ahead of it or was lost."""
    t, d = batches(k)
    return fn(k, path, pre, d.buf + t.buf)


for _name, (_k, _path, _pre) in TABLES.items():
    _case(f"count_table-{_name}", lambda k=_k, p=_path, e=_pre: _table_answer(k, p, e, batches(k)[0].buf),
          decoy=lambda k=_k, p=_path, e=_pre: _table_answer(k, p, e, batches(k)[1].buf),
          clobber=lambda k=_k, p=_path, e=_pre: _table_answer(k, p, e, clobber_bytes(batches(k)[0].n)),
          reset_lost=lambda k=_k, p=_path, e=_pre: _both(k, p, e, _table_answer))

# a second, larger count_device queued while the first is pending: MaterialiseScratch.ensure (ntk_consumer.hpp) regrows under it
GROW_COUNT_READS = (0x5EED59, 0, 400, 150, 6)   # 60 400 bytes against about 6 KB: grow_exact has to replace all three arrays


def _grown(fn):
    t, _ = batches(21)
    return fn(21, BYTES, NORMALIZE, t.buf + O.synth_reads(*GROW_COUNT_READS).tobytes())


_case("count_table_scratch_grows", lambda: _grown(_table_answer),
      first_lost=lambda: _table_answer(21, BYTES, NORMALIZE, O.synth_reads(*GROW_COUNT_READS).tobytes()),
      second_lost=lambda: _table_answer(21, BYTES, NORMALIZE, batches(21)[0].buf))


def _sketch_answer(k, path, pre, buf):
    import _sketch_model as SK
    keys = keys_answer(buf, k, path, pre)
    return {"registers": SK.registers(keys), "n_windows": int(keys.shape[0])}


_case("kmer_sketch", lambda: _sketch_answer(21, BYTES, NORMALIZE, batches(21)[0].buf),
      decoy=lambda: _sketch_answer(21, BYTES, NORMALIZE, batches(21)[1].buf),
      clobber=lambda: _sketch_answer(21, BYTES, NORMALIZE, clobber_bytes(batches(21)[0].n)),
      reset_lost=lambda: _both(21, BYTES, NORMALIZE, _sketch_answer))
_case("kmer_sketch_scratch_grows", lambda: _grown(_sketch_answer),
      first_lost=lambda: _sketch_answer(21, BYTES, NORMALIZE, O.synth_reads(*GROW_COUNT_READS).tobytes()),
      second_lost=lambda: _sketch_answer(21, BYTES, NORMALIZE, batches(21)[0].buf))

MINHASH = dict(scaled=2)


def _minhash_answer(buf):
    import _minhash_model as MH
    keys = keys_answer(buf, 21, BYTES, NORMALIZE)
    h, c = MH.sketch(keys, **MINHASH)
    return {"hashes": h, "counts": c, "n_windows": int(keys.shape[0])}


_case("minhash", lambda: _minhash_answer(batches(21)[0].buf), decoy=lambda: _minhash_answer(batches(21)[1].buf),
      clobber=lambda: _minhash_answer(clobber_bytes(batches(21)[0].n)),
      reset_lost=lambda: _minhash_answer(batches(21)[1].buf + batches(21)[0].buf))



def _merges_answer(merged: bool = True):
    """A HyperLogLog sketch and a MinHash sketch of the true batch after each folded in the decoy batch's sketch from host arrays."""
    import _minhash_model as MH
    import _sketch_model as SK
    t, d = batches(21)
    kt, kd = keys_answer(t.buf, 21, BYTES, NORMALIZE), keys_answer(d.buf, 21, BYTES, NORMALIZE)
    both = np.concatenate([kt, kd]) if merged else kt
    h, c = MH.sketch(both, **MINHASH)
    return {"registers": SK.registers(both), "sketch_n_windows": int(both.shape[0]), "hashes": h, "counts": c, "minhash_n_windows": int(both.shape[0])}


_case("host_merges", _merges_answer, merge_lost=lambda: _merges_answer(False))

# the coloured index: three colours; the true list under colour 0, then per-key masks for every other key of it
N_COLORS = 3


def color_lists(which: str):
    """(keys of the list, keys and masks of the per-key add) a colours case adds: the distinct k-mers of the true or the decoy batch,
    cut to one common length; the masks hold bits of colours 1 and 2, and - every third - a bit beyond the index's colours."""
    t, d = batches(21)
    kt, kd = items_answer(t.buf, 21, BYTES, NORMALIZE)[0], items_answer(d.buf, 21, BYTES, NORMALIZE)[0]
    n = min(kt.size, kd.size)
    keys = (kt if which == "true" else kd)[:n]
    if which == "decoy":
        keys = keys.copy()
        keys[-1] = keys[0]   # (keys may repeat: the decoy holds one key fewer)
    if which == "clobber":
        keys = np.zeros(n, dtype=np.uint64)
    sub = keys[::2].copy()
    masks = np.where(np.arange(sub.size) % 3 == 2, np.uint64(0b1110), np.where(np.arange(sub.size) % 3 == 1, np.uint64(0b110), np.uint64(0b010)))
    if which == "decoy":
        masks = np.full(sub.size, 0b1100, dtype=np.uint64)
    if which == "clobber":
        masks = np.zeros(sub.size, dtype=np.uint64)
    return keys, sub, masks.astype(np.uint64)


def color_queries() -> np.ndarray:
    """What the cases look up: every key of the true and of the decoy lists, the all-A key and one key of neither."""
    return np.unique(np.concatenate([color_lists("true")[0], color_lists("decoy")[0], np.array([0, M64 >> 22], dtype=np.uint64)]))


def _colors_index(which: str, both: bool = False):
    import _colors_model as KM
    m = KM.Index(N_COLORS)
    for w in (("decoy", which) if both else (which,)):
        keys, sub, masks = color_lists(w)
        m.add(keys, 1)
        m.add(sub, masks)
    return m


def _colors_add_answer(which: str, both: bool = False):
    m = _colors_index(which, both)
    return {"lookup": m.lookup(color_queries()), "n_keys": m.n_keys, "n_masked_bits": m.n_masked_bits, "per_color": m.per_color()}


_case("colors_add", lambda: _colors_add_answer("true"), decoy=lambda: _colors_add_answer("decoy"), clobber=lambda: _colors_add_answer("clobber"),
      reset_lost=lambda: _colors_add_answer("true", both=True))


def _views(which: str):
    """(buf, qual, offsets) a batch-and-offsets call sees: the true ones, the decoy's (all-zero offsets), or the clobber's."""
    t, d = batches(21)
    if which == "true":
        return t.buf, t.qual, t.offsets
    if which == "decoy":
        return d.buf, d.qual, np.zeros_like(t.offsets)
    if which == "clobber":
        return clobber_bytes(t.n), _zero_qual(t.n), np.zeros_like(t.offsets)
    if which == "offsets_decoy":   # the true batch under the decoy's offsets: the host, or a kernel, read the offsets early
        return t.buf, t.qual, np.zeros_like(t.offsets)
    raise KeyError(which)


ABUNDANCE_MIN_COUNT = 2
TRIM = dict(mode=1, min_count=1, min_length=0)   # NTK_TRIM_LONGEST


def _abundance_answer(which: str):
    import _abundance_model as AM
    buf, qual, off = _views(which)
    items = items_answer(buf, 21, BYTES, NORMALIZE)   # the table counted this very batch on the stream, without the quality stream
    return {"rows": AM.rows(records_of(buf, off), items, 21, BYTES, NORMALIZE, ABUNDANCE_MIN_COUNT, quals_of(qual, off), CUTOFF)}


_case("read_abundance", lambda: _abundance_answer("true"), decoy=lambda: _abundance_answer("decoy"), clobber=lambda: _abundance_answer("clobber"),
      offsets_decoy=lambda: _abundance_answer("offsets_decoy"))


def _trim_answer(which: str):
    import _trim_model as TM
    buf, qual, off = _views(which)
    items = items_answer(buf, 21, BYTES, NORMALIZE)
    recs, quals = records_of(buf, off), quals_of(qual, off)
    rows = TM.rows(recs, items, 21, BYTES, NORMALIZE, TRIM["mode"], TRIM["min_count"], TRIM["min_length"], quals, CUTOFF)
    seq, n_bytes, o_off, src, aux = TM.compact(recs, rows, quals, [0xFF] * len(recs))
    return {"rows": rows, "n_bytes": int(n_bytes), "seq": np.frombuffer(seq, dtype=np.uint8), "offsets": np.asarray(o_off, dtype=np.uint64),
            "source": np.asarray(src, dtype=np.uint64), "aux": np.frombuffer(aux, dtype=np.uint8)}


_case("read_trim", lambda: _trim_answer("true"), decoy=lambda: _trim_answer("decoy"), clobber=lambda: _trim_answer("clobber"),
      offsets_decoy=lambda: _trim_answer("offsets_decoy"))

RMH = dict(num=16)


def _rmh_answer(which: str):
    import _record_minhash_model as RM
    buf, qual, off = _views(which)
    o, w, h, c = RM.sketches(records_of(buf, off), 21, BYTES, NORMALIZE, quals=quals_of(qual, off), cutoff=CUTOFF, **RMH)
    return {"offsets": o, "n_windows": w, "hashes": h, "counts": c}


_case("record_minhash", lambda: _rmh_answer("true"), decoy=lambda: _rmh_answer("decoy"), clobber=lambda: _rmh_answer("clobber"),
      offsets_decoy=lambda: _rmh_answer("offsets_decoy"))


def _colors_screen_answer(which: str):
    import _colors_model as KM
    buf, qual, off = _views(which)
    index = _colors_index("true")   # the index is complete before the case starts
    rows, hits, single = KM.screen(records_of(buf, off), index, 21, BYTES, NORMALIZE, quals_of(qual, off), CUTOFF)
    q = color_queries() if which == "true" else (color_queries() ^ np.uint64(1) if which == "decoy" else np.zeros_like(color_queries()))
    return {"rows": rows, "hits": hits, "single": single, "lookup": index.lookup(q)}


_case("colors_screen", lambda: _colors_screen_answer("true"), decoy=lambda: _colors_screen_answer("decoy"),
      clobber=lambda: _colors_screen_answer("clobber"))

# k-mer set algebra on the list extract_device wrote in the same chain (A: the true batch's) and a complete reference list (B)
KSETS = {1: 21, 2: 47}
KSET_BINS = (8, 4)


def kset_lists(words: int, which: str):
    """(A keys, A counts, B keys, B counts): A is the list of `which`, cut to the length the true and the decoy lists share; B the k-mers
    of half of the true batch's records and half of the decoy's, with their counts there plus 1."""
    k = KSETS[words]
    t, d = batches(k)
    (kt, ct), (kd, cd) = items_answer(t.buf, k, BYTES, NORMALIZE), items_answer(d.buf, k, BYTES, NORMALIZE)
    n = min(ct.size, cd.size)
    a = {"true": (kt[:n], ct[:n]), "decoy": (kd[:n], cd[:n] + np.uint64(2)),
         "clobber": (np.zeros_like(kt[:n]), np.zeros(n, dtype=np.uint64))}[which]
    ref = b"".join(r + b"\n" for r in t.records[::2] + d.records[1::2])
    kb, cb = items_answer(ref, k, BYTES, NORMALIZE)
    return a[0], a[1], kb, cb + np.uint64(1)


def _ksets_answer(words: int, which: str):
    import _kmer_sets_model as KS
    ka, ca, kb, cb = kset_lists(words, which)
    da, db = KS.as_dict(ka, ca), KS.as_dict(kb, cb)
    hist, totals = KS.compare(da, db, *KSET_BINS)
    out_k, out_c = KS.as_list(KS.apply(KS.INTERSECT, KS.MIN, da, db), words)
    uni_k, uni_c = KS.as_list(KS.apply(KS.UNION, KS.SUM, da, db), words)
    return {"hist": np.asarray(hist, dtype=np.uint64).reshape(-1), "totals": tuple(int(totals[name]) for name in KS.TOTALS),
            "intersect_keys": np.asarray(out_k), "intersect_counts": np.asarray(out_c), "union_keys": np.asarray(uni_k), "union_counts": np.asarray(uni_c)}


for _w in KSETS:
    _case(f"kmer_sets-{_w}", lambda w=_w: _ksets_answer(w, "true"), decoy=lambda w=_w: _ksets_answer(w, "decoy"))
    # validate alone takes any list: its decoy is the true list reversed, its clobber all-zero keys - n - 1 violations each
    _case(f"kmer_sets_validate-{_w}", lambda w=_w: {"violations": 0}, decoy=lambda w=_w: {"violations": kset_lists(w, "true")[0].shape[0] - 1},
          clobber=lambda w=_w: {"violations": kset_lists(w, "true")[0].shape[0] - 1})


def dbg_lists(which: str):
    """(keys, counts) of the graph's list at k = 21: the canonical k-mers of the batch, cut to the length both lists share (a prefix of
    an ascending list of canonical k-mers is one)."""
    t, d = batches(21)
    (kt, ct), (kd, cd) = items_answer(t.buf, 21, BYTES, NORMALIZE), items_answer(d.buf, 21, BYTES, NORMALIZE)
    n = min(ct.size, cd.size)
    return (kt[:n], ct[:n]) if which == "true" else (kd[:n], cd[:n] + np.uint64(2))


def _dbg_answer(which: str):
    import _dbg_model as DM
    keys, counts = dbg_lists(which)
    m = DM.Graph(keys, counts, 21)
    text, off = m.batch()
    totals = m.totals()
    recount = items_answer(bytes(text[:int(off[-1])]), 21, BYTES, NORMALIZE)
    return {"edges": np.asarray(m.edges), "totals": tuple(np.asarray(totals[key]).tolist() for key in DM.TOTALS), "n_unitigs": int(m.n_unitigs),
            "n_bases": int(m.n_bases), "kmer_rows": np.asarray(m.kmer_rows), "unitig_rows": np.asarray(m.unitig_rows),
            "text": np.asarray(text), "offsets": np.asarray(off, dtype=np.uint64), "recount_keys": recount[0]}   # (every recount is 1: asserted beside it)


_case("dbg", lambda: _dbg_answer("true"), decoy=lambda: _dbg_answer("decoy"))


# the all-pairs compare takes host inputs: there is no decoy.  Two sets of sketches; the answer is _mhset_model.block
def mhset_sketches():
    import _minhash_model as MH
    t, d = batches(21)
    out = []
    for b in (t, d):
        for recs in (b.records[:24], b.records[24:], b.records[::2]):
            out.append(MH.sketch(keys_answer(b"".join(r + b"\n" for r in recs), 21, BYTES, NORMALIZE), num=64))
    return out


def _mhset_answer():
    import _mhset_model as SM
    sk = mhset_sketches()
    return SM.block(sk, sk, 64, M64, True)


_case("mhset_compare", _mhset_answer)

# one chain like a user's: trim -> count -> extract -> intersect with the reference's list -> unitigs -> per-record sketches
CHAIN_RMH = dict(scaled=1)


def chain_answer(skip: str = None) -> dict:
    """Every stage of the chain from the models.  skip: the answer had that stage been skipped - the trim (the whole batch goes on), the
    intersection (the table's own list goes on), the graph (the sketches are the input batch's)."""
    import _dbg_model as DM
    import _kmer_sets_model as KS
    import _record_minhash_model as RM
    import _trim_model as TM
    t, d = batches(21)
    ref_items = items_answer(b"".join(r + b"\n" for r in t.records[::2] + d.records[1::2]), 21, BYTES, NORMALIZE)
    base_items = items_answer(t.buf, 21, BYTES, NORMALIZE)
    rows = TM.rows(t.records, base_items, 21, BYTES, NORMALIZE, TRIM["mode"], TRIM["min_count"], TRIM["min_length"], t.quals, CUTOFF)
    seq, n_bytes, o_off, src, aux = TM.compact(t.records, rows, t.quals, [0xFF] * len(t.records))
    kept = t.buf if skip == "trim" else bytes(seq[:n_bytes])
    keys, counts = items_answer(kept, 21, BYTES, NORMALIZE)
    da, db = KS.as_dict(keys, counts), KS.as_dict(*ref_items)
    joined = da if skip == "intersect" else KS.apply(KS.INTERSECT, KS.LEFT, da, db)
    jk, jc = KS.as_list(joined, 1)
    g = DM.Graph(np.asarray(jk, dtype=np.uint64), np.asarray(jc, dtype=np.uint64), 21)
    text, off = g.batch()
    spelled = t.records if skip == "graph" else [u.encode() for u in g.spelled]
    o, w, h, c = RM.sketches(spelled, 21, BYTES, NORMALIZE, **CHAIN_RMH)
    return {"trim_rows": rows, "kept": np.frombuffer(kept, dtype=np.uint8), "table_keys": keys, "table_counts": counts,
            "joined_keys": np.asarray(jk, dtype=np.uint64), "joined_counts": np.asarray(jc, dtype=np.uint64), "unitig_rows": np.asarray(g.unitig_rows),
            "unitig_text": np.asarray(text), "sketch_offsets": o, "sketch_hashes": h, "sketch_counts": c}


CHAIN_AFTER = {"trim": ("kept", "table_keys", "table_counts", "joined_keys", "joined_counts", "unitig_rows", "unitig_text", "sketch_offsets", "sketch_hashes", "sketch_counts"),
               "intersect": ("joined_keys", "joined_counts", "unitig_rows", "unitig_text", "sketch_offsets", "sketch_hashes", "sketch_counts"),
               "graph": ("sketch_offsets", "sketch_hashes", "sketch_counts")}
_case("chain", chain_answer)

_case("negative_control", lambda: {"sum": int(np.frombuffer(batches(21)[0].buf, dtype=np.uint8).sum(dtype=np.int64))},
      decoy=lambda: {"sum": int(np.frombuffer(batches(21)[1].buf, dtype=np.uint8).sum(dtype=np.int64))})
