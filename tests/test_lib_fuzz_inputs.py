"""The slices of tests/test_gpu_lib_fuzz.py are not vacuous: proved here without a GPU, from the generator (tests/_lib_fuzz.py) and the
host models alone, over the exact seeds and case counts the GPU tests use (`_lib_fuzz.SLICES`).  These are conditions, not
measurements: when one fails, the generator changes, not the condition."""
import functools

import numpy as np
import pytest

import oracle as O  # the checker
import _abundance_model as A
import _colors_model as KM
import _kmer_sets_model as KS
import _lib_fuzz as F
import _minhash_model as M
import _record_minhash_model as RM
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
        if stage in F.WIDE_STAGES:
            assert c.k in F.WIDE_KS and c.path == F.BYTES and c.pre in F.WIDE_PRES
        elif stage == "dbg":   # odd k on a canonical path
            assert c.k in F.DBG_KS and c.k % 2 == 1 and (c.path, c.pre) in F.PATH_PRES and c.path != F.BITS
        else:
            assert c.k in F.KS and (c.path, c.pre) in F.PATH_PRES
        assert c.stage == (stage if stage in F.NEW_STAGES else "count") and c.extra == c2.extra


# SHA-256 of the six first slices (`_lib_fuzz.slice_digest`), taken on the commit before the five newer stages were added: the generator
# still makes, byte for byte, the cases it made then
PINNED = {"count": "0bfdd272af60d3de0dbc8f7830998dd5a5e1e1fa6b6d7e68dace584ca0dec73a",
          "count_wide": "8a553be815c6873d8d7fad9e152c65d06da7e80407aecb4a0c3967610744e2e0",
          "minhash": "91db4499f988dfd9f8edd3c102562ddbcdd7308fa675869e5add759054eabd42",
          "minhash_wide": "689f06eae7768e6f532e979f903c98ba31d56730baa4bfb913499b8eb7e6b004",
          "abundance": "f07215e94d578b8b69bfe2252fdbeea9b038070f3778e15c22f7c24b845a25c0",
          "trim": "3668c86e92983f7dc60b78704c43e414ed4a0c7d7427019cbea4d9322d6eaeac"}
PINNED_SLICES = {"count": (103, 3), "count_wide": (111, 3), "minhash": (134, 8), "minhash_wide": (131, 10), "abundance": (104, 3),
                 "trim": (111, 4)}


@pytest.mark.parametrize("stage", F.OLD_STAGES)
def test_the_six_first_slices_are_byte_for_byte_what_they_were(stage):
    assert set(PINNED) == set(F.OLD_STAGES) and F.STAGES[:6] == F.OLD_STAGES   # a stage's index seeds its cases
    assert F.SLICES[stage] == PINNED_SLICES[stage]
    assert F.slice_digest(stage) == PINNED[stage]
    assert F.edge_lengths(21, stage) == F.edge_lengths(21) and F.long_classes(stage) == F.LONG_CLASSES


@pytest.mark.parametrize("stage", F.STAGES)
def test_every_content_kind_and_edge_length_occurs(stage):
    kinds, classes, residues = set(), set(), set()
    one_below = one_above = 0
    for _, c in cases(stage):
        kinds |= set(c.kinds)
        classes |= {x for x in c.classes if x is not None}
        residues |= set((c.starts() % 16).tolist())
        lengths = F.edge_lengths(c.k, c.stage, c.num())
        for r, cls, kind in zip(c.records, c.classes, c.kinds):   # a class is the length it names
            if cls in lengths:
                assert len(r) == lengths[cls]
            elif cls == "long_pieces":
                assert abs(len(r) - F.LONG_PIECES_BYTES) <= 17
            elif cls == "long_record":
                assert abs(len(r) - c.k + 1 - F.LONG_RECORD) <= 1
            elif cls == F.COLORS_LONG:   # genome content: every candidate window is a k-mer, or is cut by a drawn break
                assert abs(len(r) - c.k + 1 - KM.LONG_RECORD) <= 1 and kind not in ("clean", "periodic")
            elif cls in F.TAU_CLASSES:
                assert len(r) == (32 if cls == "tau_alone" else F.TAU_INSIDE) and c.k == 32 and "scaled" in c.extra["kind"]
            else:
                assert cls is None
        assert all(sum(x == name for x in c.classes) <= 1 for name in F.ALL_LONG_CLASSES)
        assert {x for x in c.classes if x in F.ALL_LONG_CLASSES} <= set(F.long_classes(stage))
        assert sum(len(r) for r, cls in zip(c.records, c.classes) if cls not in F.ALL_LONG_CLASSES) < 24_000 + \
            (F.RMH_EDGE_MAX if stage == "record_minhash" else 0)   # "about 20 KB", and at most one more record of the longest class
        deleted = set(F.DELETED[c.pre])
        assert not any(deleted & set(r) for r in c.records)   # the excluded byte class
        q, base = c.qual_stream(), c.cutoff if c.cutoff else 40
        one_below += int((q == base - 1).sum())
        one_above += int((q == base + 1).sum())
    assert kinds >= set(F.KINDS), set(F.KINDS) - kinds
    want = set(F.edge_lengths(21, stage)) | set(F.long_classes(stage))
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


# ---- the five newer stages ------------------------------------------------------------------------------------------------------------

ALL = M.ALL


def rmh_guess(n_ends: int, num: int) -> int:
    """rmh_guess of needletail_amd/csrc/ntk_rmh_rule.hpp, restated (tests/test_rmh_rule.py holds the header to the same text)."""
    if n_ends <= 4 * num or n_ends <= F.rmh_want(num):
        return ALL
    return (ALL // n_ends) * F.rmh_want(num)


def rmh_accept(tau: int, distinct: int, num: int) -> bool:
    return tau == ALL or distinct >= num


def record_minhash_report():
    r = dict(allpass=0, guessed=0, raised=0, overflow=0, tile3=0, start256=0, small=0, large=0, scaled1=0, num1=0, edge_below=0,
             edge_above=0, at_tau_start=0, at_tau_inside=0)
    for rng, c in cases("record_minhash"):
        kind, buffer_entries = c.extra["kind"], c.extra["buffer_entries"]
        d = F.draw_rmh(_copy(rng), c)
        values = F.rmh_values(c, True)   # the call whose result becomes the set
        off, _, hashes, counts = RM.csr(values, **kind)
        sizes = np.diff(off.astype(np.int64))
        ends = np.array([max(len(x) - c.k + 1, 0) for x in c.records])   # candidate window ends: hi - lo of record_span
        if "num" in kind:
            num = kind["num"]
            r["num1"] += num == 1
            r["allpass"] += int(((ends > 0) & (ends <= 4 * num)).sum())
            r["guessed"] += int((ends > 4 * num).sum())
            r["edge_below"] += sum(x in ("4num-1", "4num") for x in c.classes)
            r["edge_above"] += sum(x == "4num+1" for x in c.classes)
            for v, n_ends in zip(values, ends):
                tau = rmh_guess(int(n_ends), num)
                if tau != ALL and v.size:
                    distinct = int((np.unique(M.S.hash_keys(v)) <= np.uint64(tau)).sum())
                    r["raised"] += not rmh_accept(tau, distinct, num)
        else:
            r["scaled1"] += kind["scaled"] == 1 and hashes.size > 0
            # A hash that IS the threshold max_hash(scaled), which the filter's <= keeps: in a 256-end tile of the batch that holds a
            # record start (every lane finds its own record there) and in a tile inside one record (the uniform path).  The tiles are
            # those of a launch over the whole batch, which is what a run is unless it is redone in pieces
            off_b = c.offsets().astype(np.int64)
            for i, v in enumerate(F.rmh_values(c, False)):
                if v.size and (M.S.hash_keys(v) == np.uint64(M.max_hash(kind["scaled"]))).any():
                    assert c.classes[i] in F.TAU_CLASSES and v.size == len(c.records[i]) - c.k + 1   # no break: window j ends at byte j + k - 1
                    j = int(np.flatnonzero(M.S.hash_keys(v) == np.uint64(M.max_hash(kind["scaled"])))[0])
                    tile = (int(off_b[i]) + j + c.k - 1) // 256
                    holds_start = bool(((off_b >= tile * 256) & (off_b < tile * 256 + 256)).any())
                    r["at_tau_start" if holds_start else "at_tau_inside"] += 1
        # every occurrence of a kept hash passed the filter: at least that many pairs in the call
        r["overflow"] += buffer_entries > 0 and int(counts.sum()) > buffer_entries
        starts = c.starts()
        tiles = {}
        for i, (s, n_ends) in enumerate(zip(starts, ends)):   # the 256-end tiles of the batch that hold a window end of record i
            if n_ends:
                for t in range(int(s + c.k - 1) // 256, int(s + c.k - 1 + n_ends - 1) // 256 + 1):
                    tiles.setdefault(t, set()).add(i)
        r["tile3"] += any(len(v) >= 3 for v in tiles.values())
        r["start256"] += int(((starts % 256 == 0) & (ends > 0)).sum())
        r["small"] += int(((sizes > 0) & (sizes <= 2048)).sum())
        r["large"] += int((sizes > 2048).sum())
        assert 1 <= d["prefix"] <= len(c.records)
    return r


def test_record_minhash_slice_meets_both_sides_of_its_rules():
    r = record_minhash_report()
    assert r["allpass"] >= 1 and r["guessed"] >= 1, r         # records at or below the all-pass length 4 num, and above it
    assert r["edge_below"] >= 1 and r["edge_above"] >= 1, r   # and the edge lengths on both sides of it
    assert r["raised"] >= 1, r                                # a first guess that is rejected and raised
    assert r["overflow"] >= 1, r                              # more passing hashes than buffer_entries: the launch is redone in pieces
    assert r["tile3"] >= 1 and r["start256"] >= 1, r          # three records in one 256-end tile; a record that starts a tile
    assert r["small"] >= 1 and r["large"] >= 1, r             # sketches on both sides of the sketch set's 2048-hash LDS stage
    assert r["scaled1"] >= 1 and r["num1"] >= 1, r
    assert r["at_tau_start"] >= 1 and r["at_tau_inside"] >= 1, r   # a hash equal to the threshold, on both paths of the filter


def kmer_sets_report(stage):
    r = dict(three_way=0, differ=0, tiles=0, min_count=0, chained=0)
    tile = KS.TILE_WORDS // (2 if stage == "kmer_sets_wide" else 1)
    for rng, c in cases(stage):
        d = F.draw_ksets(_copy(rng))
        da, db = F.ksets_operands(c, d)
        t = KS.compare(da, db, 2, 2)[1]
        r["three_way"] += t["n_shared"] > 0 and t["n_a_only"] > 0 and t["n_b_only"] > 0
        r["differ"] += any(db.get(key, v) != v for key, v in da.items())
        r["tiles"] += len(da) + len(db) > 3 * tile
        r["min_count"] += d["mc_a"] > 1 or d["mc_b"] > 1
        r["chained"] += len(F.ksets_chain(d, da, db)) > 0
    return r


@pytest.mark.parametrize("stage", ["kmer_sets", "kmer_sets_wide"])
def test_kmer_sets_slice_has_all_three_parts_and_more_than_three_tiles(stage):
    r = kmer_sets_report(stage)
    assert r["three_way"] >= 1, r   # shared keys, keys of the first set only, keys of the second only
    assert r["differ"] >= 1, r      # a shared key with two counts: the rules differ
    assert r["tiles"] >= 1, r       # the merged length is above three tiles
    assert r["min_count"] >= 1 and r["chained"] >= 1, r


def dbg_report():
    r = dict(cycles=0, isolated=0, tips=0, branching=0, self_loops=0, one=0, long=0, k31=0, k3=0, fed=[])
    for rng, c in cases("dbg"):
        d = F.draw_dbg(_copy(rng))
        keys, counts, m = F.dbg_graph(c, d)
        t = m.totals()
        r["cycles"] += int((m.unitig_rows[:, 3] & np.uint64(1)).sum())
        r["isolated"] += t["n_isolated"]
        r["tips"] += t["n_tips"]
        r["branching"] += t["n_branching"]
        r["self_loops"] += t["n_self"]
        r["one"] += int((m.unitig_rows[:, 1] == 1).sum())
        r["long"] += int((m.unitig_rows[:, 1] > 64).sum())
        r["k31"] += c.k == 31
        r["k3"] += c.k == 3
        r["fed"].append(m.n_unitigs)
        assert [x for x in c.ref_records[-2:]] == [bytes(np.resize(np.frombuffer(u, dtype=np.uint8), len(x)))
                                                   for u, x in zip(F.DBG_UNITS, c.ref_records[-2:])]
    return r


def test_dbg_slice_has_every_shape_of_a_graph():
    r = dbg_report()
    for name in ("cycles", "isolated", "tips", "branching", "self_loops", "one", "long", "k31", "k3"):
        assert r[name] >= 1, (name, r)
    assert min(r["fed"]) > 0, r   # every case's unitig batch has records to feed on: none is left out


def colors_report():
    r = dict(routes=set(), n_colors=set(), absent=0, single=0, tie=0, no_second=0, no_hit=0, masked_bits=0, dead=0, windows=set(),
             cut_left=0, cut_right=0, fed=[], star=0)
    for rng, c in cases("colors"):
        d = F.draw_colors(_copy(rng), c)
        model, steps = F.colors_steps(c, d)
        r["routes"] |= {s[0] for s in steps if s[1] is not None}
        r["n_colors"].add(d["n_colors"])
        r["star"] += d["star"] is not None
        r["masked_bits"] += model.n_masked_bits
        rows, hits, single = KM.screen_values(F.colors_values(c, False), model)
        some = rows[:, 0] > 0
        r["absent"] += int((rows[:, 1] < rows[:, 0]).sum())
        r["single"] += int((rows[:, 2] > 0).sum())
        for row, h in zip(rows, hits):
            b = int(row[3])
            if b != KM.NONE:
                r["tie"] += bool((h[b + 1:] == h[b]).any())
                r["no_second"] += int(row[4]) == KM.NONE
        r["no_hit"] += int((some & (rows[:, 3] == np.uint64(KM.NONE))).sum())
        if d["dead"] is not None:   # its k-mers were added, with no bit below n_colors, and nothing else of it is in the index
            r["dead"] += int(rows[d["dead"], 0]) > 0 and int(rows[d["dead"], 1]) == 0
        r["windows"] |= {len(x) - c.k + 1 for x in c.records}
        items = oracle_items(pack(c.ref_records), c.k, c.path, c.pre)
        fed, want = F.trim_chain(c, items, d["trim"])
        L = np.array([len(x) for x in c.records], dtype=np.uint64)
        kept = fed[:, 1] > 0
        r["cut_left"] += int((kept & (fed[:, 0] > 0)).sum())
        r["cut_right"] += int((kept & (fed[:, 0] + fed[:, 1] < L)).sum())
        r["fed"].append(int(kept.sum()))
        assert len(want[3]) == int(kept.sum())
    return r


def test_colors_slice_meets_both_sides_of_its_rules():
    r = colors_report()
    assert r["routes"] == set(F.ROUTES), r                      # a table, a set and per-key masks
    assert 64 in r["n_colors"] and min(r["n_colors"]) < 3, r
    assert r["star"] >= 1, r                                    # a colour whose hits are held to ReadAbundance on its table
    assert r["absent"] >= 1 and r["single"] >= 1, r             # rows with n_hit < n_kmers, rows with n_single > 0
    assert r["tie"] >= 1, r                                     # best is a tie that goes to the lower colour
    assert r["no_second"] >= 1 and r["no_hit"] >= 1, r
    assert r["masked_bits"] >= 1 and r["dead"] >= 1, r          # a mask loses a bit; a record hits only keys that were added without a colour
    assert {KM.LONG_RECORD, KM.LONG_RECORD + 1} <= r["windows"], sorted(w for w in r["windows"] if w > 10000)
    assert r["cut_left"] >= 1 and r["cut_right"] >= 1, r        # the compacted batch that is fed back has records cut on each side
    assert min(r["fed"]) > 0, r                                 # and every case feeds one back
