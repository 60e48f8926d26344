"""The slices of tests/test_gpu_lib_fuzz.py are not vacuous: proved here without a GPU, from the generator (tests/_lib_fuzz.py) and the
host models alone, over the exact seeds and case counts the GPU tests use (`_lib_fuzz.SLICES`).  These are conditions, not
measurements: when one fails, the generator changes, not the condition."""
import functools

import numpy as np
import pytest

import oracle as O  # the checker
import _abundance_model as A
import _lib_fuzz as F
import _minhash_model as M
import _trim_model as T
from _count_helpers import oracle_items, pack


@functools.lru_cache(maxsize=None)
def cases(stage):
    seed, n = F.SLICES[stage]
    return tuple(F.draw_case(seed, stage, it) for it in range(1, n + 1))   # (rng after the case, case)


@pytest.mark.parametrize("stage", F.STAGES)
def test_the_generator_is_deterministic_and_nothing_is_left_out(stage):
    seed, n = F.SLICES[stage]
    got = cases(stage)
    assert len(got) == n   # every iteration is a case: nothing is skipped or filtered after generation, the share left out is 0
    for it, (rng, c) in enumerate(got, 1):
        rng2, c2 = F.draw_case(seed, stage, it)
        assert (c.k, c.path, c.pre, c.cutoff) == (c2.k, c2.path, c2.pre, c2.cutoff)
        assert c.records == c2.records and c.ref_records == c2.ref_records and c.kinds == c2.kinds and c.classes == c2.classes
        assert np.array_equal(c.qual_stream(), c2.qual_stream())
        assert rng.bit_generator.state == rng2.bit_generator.state   # and so are the checker's draws that follow
        assert len(c.records) > 0 and len(c.ref_records) > 0
        assert c.cutoff == 0 or 33 <= c.cutoff <= 75
        assert (c.k in F.WIDE_KS and c.path == F.BYTES and c.pre in F.WIDE_PRES) if stage in F.WIDE_STAGES else \
            (c.k in F.KS and (c.path, c.pre) in F.PATH_PRES)


@pytest.mark.parametrize("stage", F.STAGES)
def test_every_content_kind_and_edge_length_occurs(stage):
    kinds, classes, residues = set(), set(), set()
    one_below = one_above = 0
    for _, c in cases(stage):
        kinds |= set(c.kinds)
        classes |= {x for x in c.classes if x is not None}
        residues |= set((c.starts() % 16).tolist())
        lengths = F.edge_lengths(c.k)
        for r, cls in zip(c.records, c.classes):   # a class is the length it names
            if cls in lengths:
                assert len(r) == lengths[cls]
            elif cls == "long_pieces":
                assert abs(len(r) - F.LONG_PIECES_BYTES) <= 17
            elif cls == "long_record":
                assert abs(len(r) - c.k + 1 - F.LONG_RECORD) <= 1
        assert sum(x == "long_pieces" for x in c.classes) <= 1 and sum(x == "long_record" for x in c.classes) <= 1
        assert sum(len(r) for r, cls in zip(c.records, c.classes) if cls not in F.LONG_CLASSES) < 24_000   # "about 20 KB"
        deleted = set(F.DELETED[c.pre])
        assert not any(deleted & set(r) for r in c.records)   # the excluded byte class
        q, base = c.qual_stream(), c.cutoff if c.cutoff else 40
        one_below += int((q == base - 1).sum())
        one_above += int((q == base + 1).sum())
    assert kinds >= set(F.KINDS), set(F.KINDS) - kinds
    want = set(F.edge_lengths(21)) | set(F.LONG_CLASSES)
    assert classes >= want, want - classes
    assert residues == set(range(16))   # a record starts at every offset of the 16-byte copy piece
    assert one_below > 0 and one_above > 0   # both sides of the cutoff's <


def abundance_report():
    nonempty = apart = three = 0
    windows = set()
    for _, c in cases("abundance"):
        items = oracle_items(pack(c.ref_records), c.k, c.path, c.pre)
        rows = A.rows(c.records, items, c.k, c.path, c.pre)
        ne = rows[:, 0] > 0
        nonempty += int(ne.sum())
        apart += int((ne & (rows[:, 2] < rows[:, 4])).sum())
        three += int((ne & (rows[:, 2] < rows[:, 3]) & (rows[:, 3] < rows[:, 4])).sum())
        windows |= {len(r) - c.k + 1 for r in c.records}
    return dict(nonempty=nonempty, apart=apart, three=three, windows=windows)


def test_abundance_slice_has_statistics_that_differ():
    r = abundance_report()
    assert r["nonempty"] > 0 and 4 * r["apart"] >= r["nonempty"], r   # min < max in a quarter of the non-empty rows
    assert r["three"] >= 1                                              # min < median < max
    assert 192 in r["windows"] and 193 in r["windows"]                 # kRegWindows and the first record past it


def trim_report():
    nonempty = 0
    cut = {m: 0 for m in F.MODES}
    disagree, residues, fed_back = 0, set(), []
    for rng, c in cases("trim"):
        items = oracle_items(pack(c.ref_records), c.k, c.path, c.pre)
        wins = [T.record_windows(r, c.k, c.path, c.pre) for r in c.records]
        L = np.array([len(r) for r in c.records], dtype=np.uint64)
        rows = {m: T.rows_from_windows(c.records, wins, items, c.k, m) for m in F.MODES}
        nonempty += int((L > 0).sum())
        for m in F.MODES:
            kept = rows[m][:, 1] > 0
            cut[m] += int((kept & (rows[m][:, 1] < L)).sum())
            residues |= set(((c.starts()[kept] + rows[m][kept, 0].astype(np.int64)) % 16).tolist())
        disagree += int((rows[T.PREFIX][:, :2] != rows[T.LONGEST][:, :2]).any(axis=1).sum())
        # the setting the checker compacts and feeds back (its draws follow the case's), with the quality mask
        mode, mc, ml = F.draw_trim(_copy(rng), c.k)
        fed = T.rows(c.records, items, c.k, c.path, c.pre, mode, mc, ml, c.quals, c.cutoff)
        fed_back.append(int((fed[:, 1] > 0).sum()))
    return dict(nonempty=nonempty, cut=cut, disagree=disagree, residues=residues, fed_back=fed_back)


def _copy(rng):
    """A generator in the same state: the checker's draws without disturbing the cached one."""
    g = np.random.default_rng()
    g.bit_generator.state = rng.bit_generator.state
    return g


def test_trim_slice_cuts_records_in_both_modes():
    r = trim_report()
    for m in F.MODES:
        assert 4 * r["cut"][m] >= r["nonempty"], r   # a kept interval that is neither empty nor the whole record
    assert r["disagree"] >= 1
    assert r["residues"] == set(range(16))            # a kept interval starts at every residue of the 16-byte copy piece
    assert min(r["fed_back"]) > 0, r                  # every case's round trip has records to feed back: none is left out


def late_tie(c, kind, use_q, pieces, ops) -> bool:
    """A repeat of the threshold hash arrives after the threshold was fixed there: before some call j >= 1 the handle holds num hashes
    and was made to fold its buffer (an observing call after call j - 1; cases that merge are not counted), call j adds a key whose hash IS that
    threshold, and the threshold is still there at the end - so the count of the num-th hash is only right if the filter's compare
    is <=.  (A reset only starts the same calls over.)"""
    if "num" not in kind or "merge" in ops:
        return False
    buf, qual, cuts = F.split_records(c, pieces)
    masked = F.quality_masked(buf, qual, c.cutoff) if use_q else buf
    per_call = [F.oracle_keys(masked[a:b], c.k, c.path, c.pre) for a, b in zip(cuts[:-1], cuts[1:])]
    final = M.sketch(np.concatenate(per_call), **kind)[0]
    if final.size < kind["num"]:
        return False
    for j in range(1, len(per_call)):
        before = M.sketch(np.concatenate(per_call[:j]), **kind)[0]
        if ops[j - 1] != "nothing" and before.size == kind["num"] and before[-1] == final[-1] and \
                (M.S.hash_keys(per_call[j]) == final[-1]).any():
            return True
    return False


def minhash_report(stage):
    more = fewer = overflow = tie = late = scaled1 = merges = resets = 0
    for rng, c in cases(stage):
        kind, buffer_entries, use_q, pieces, ops, reset_after = F.draw_minhash(_copy(rng))
        keys = F.oracle_keys(F.masked_buf(c, use_q), c.k, c.path, c.pre)
        distinct = np.unique(keys, axis=0).shape[0] if keys.shape[0] else 0
        h, cnt = M.sketch(keys, **kind)
        if "num" in kind:
            more += distinct > kind["num"]
            fewer += 0 < distinct < kind["num"]
            tie += h.size >= kind["num"] and int(cnt[kind["num"] - 1]) > 1
        else:
            scaled1 += kind["scaled"] == 1 and h.size > 0
        late += late_tie(c, kind, use_q, pieces, ops)
        overflow += buffer_entries > 0 and int(cnt.sum()) > buffer_entries   # hashes at or below the final threshold passed every filter
        merges += "merge" in ops
        resets += reset_after >= 0
    return dict(more=more, fewer=fewer, overflow=overflow, tie=tie, late_tie=late, scaled1=scaled1, merges=merges, resets=resets)


@pytest.mark.parametrize("stage", ["minhash", "minhash_wide"])
def test_minhash_slice_meets_both_sides_of_its_rules(stage):
    r = minhash_report(stage)
    assert r["more"] >= 1 and r["fewer"] >= 1, r   # more distinct keys than num, and fewer
    assert r["overflow"] >= 1, r                    # more passing hashes than buffer_entries: a launch must be redone
    assert r["tie"] >= 1, r                         # the num-th hash occurs more than once
    assert r["late_tie"] >= 1, r                    # and once more after the threshold was fixed at it (see late_tie)
    assert r["scaled1"] >= 1, r
    assert r["merges"] >= 1 and r["resets"] >= 1, r


def wide_window_ends(buf: bytes, k: int) -> np.ndarray:
    """The batch offsets of the last byte of every window the oracle's iterator emits (the byte path after normalize)."""
    a = np.frombuffer(buf, dtype=np.uint8)
    base = np.isin(a, np.frombuffer(b"ACGTacgtUu", dtype=np.uint8))
    norm = O.normalize(np.where(base, a, ord("N")).astype(np.uint8).tobytes())[0]
    pos, _ = O.canonical_kmers_arrays(norm, O.reverse_complement(norm), k)
    return pos.astype(np.int64) + (k - 1)


@pytest.mark.parametrize("stage", F.WIDE_STAGES)
def test_wide_slices_have_windows_on_both_sides_of_a_lane_run_boundary(stage):
    last = first = near = 0
    for _, c in cases(stage):
        ends = wide_window_ends(c.buf(), c.k)
        assert ends.size == F.oracle_keys(c.buf(), c.k, c.path, c.pre).shape[0]
        last += int((ends % F.LANE_RUN == F.LANE_RUN - 1).sum())
        first += int((ends % F.LANE_RUN == 0).sum())
        # a record or a run of bases that starts within k - 1 bytes after a boundary: its first window is primed across it
        starts = ends[np.concatenate([[True], np.diff(ends) > 1])] - (c.k - 1)
        near += int((starts % F.LANE_RUN < c.k).sum())
    assert last > 0 and first > 0 and near > 0
