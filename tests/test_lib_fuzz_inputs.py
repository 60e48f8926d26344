"""The slices of tests/test_gpu_lib_fuzz.py are not vacuous: proved here without a GPU, from the generator (tests/_lib_fuzz.py) and the
host models alone, over the exact seeds and case counts the GPU tests use (`_lib_fuzz.SLICES`).  These are conditions, not
measurements: when one fails, the generator changes, not the condition.  Thirteen stages over sixteen libraries: the last, `map_reads`,
has its conditions in tests/_map_reads_report.py (seeds, chains, mappings and alignments on both sides of their rules, every CIGAR walked
independently of the model, every planted wrong rule of the four models caught)."""
import functools

import numpy as np
import pytest

import oracle as O  # the checker
import _abundance_model as A
import _colors_model as KM
import _kmer_sets_model as KS
import _lib_fuzz as F
import _minhash_model as M
import _minimizer_list_model as MM
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
        elif stage in F.PIPELINE_STAGES:   # ReadMapper's lists: the bit-canonical path, the k that leave room for seeds
            assert c.k in F.MAP_KS and c.path == F.BITS_CANON and c.pre in F.MAP_PRES and c.origins == c2.origins
        elif stage == "dbg":   # odd k on a canonical path
            assert c.k in F.DBG_KS and c.k % 2 == 1 and (c.path, c.pre) in F.PATH_PRES and c.path != F.BITS
        else:
            assert c.k in F.KS and (c.path, c.pre) in F.PATH_PRES
        assert c.stage == (stage if stage in F.NEW_STAGES + F.PIPELINE_STAGES else "count") and c.extra == c2.extra


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


@pytest.mark.parametrize("stage", F.OLD_STAGES + F.NEW_STAGES)   # (the map_reads stage has reads of its own kinds: its section below)
def test_every_content_kind_and_edge_length_occurs(stage):
    kinds, classes, residues = set(), set(), set()
    one_below = one_above = 0
    for _, c in cases(stage):
        kinds |= set(c.kinds)
        classes |= {x for x in c.classes if x is not None}
        residues |= set((c.starts() % 16).tolist())
        lengths = c.edges()
        assert lengths == F.edge_lengths(c.k, c.stage, c.num(), c.extra.get("w", 0))
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


# ---- the minimizer_list stage ------------------------------------------------------------------------------------------------------------
#
# Everything below is computed from the model alone (`_minimizer_list_model.planes` / `windows` / `csr`) on the packed batch of a case, as
# the checker's first run takes it: no quality stream, `_trim_model.offsets`.  A tile boundary is a multiple of ML_TILE window ends of
# that batch (a run starts its tiles at end 0: one chunk).

def test_the_minimizer_list_tile_is_the_rules():
    rule = open(F.MM.__file__.replace("_minimizer_list_model.py", "../needletail_amd/csrc/ntk_ml_rule.hpp")).read()
    assert f"constexpr uint32_t ML_TILE = {F.ML_TILE};" in rule and F.ML_TILE == MM.TILE == 1024
    assert f"constexpr uint32_t ML_W_MAX = {max(max(ws) for ws in F.ML_W_CLASSES.values())};" in rule
    e = F.edge_lengths(21, "minimizer_list", window=11)
    assert (e["k+w-2"], e["k+w-1"], e["k+w"], e["k+2w-1"]) == (30, 31, 32, 42)      # no window, one, two, a run of w + 1
    assert (e["T1023"], e["T1024"], e["T1025"]) == (1043, 1044, 1045)                  # ML_TILE - 1, ML_TILE, ML_TILE + 1 window ends
    assert set(e) - set(F.edge_lengths(21)) == {"k+w-2", "k+w-1", "k+w", "k+2w-1", "T1023", "T1024", "T1025"}
    assert F.long_classes("minimizer_list") == () and F.STAGES[11] == "minimizer_list" and F.STAGES[12:] == F.PIPELINE_STAGES
    for name, ws in F.ML_W_CLASSES.items():
        for w in ws:
            assert (name == "one") == (w == 1) and (name == "power_of_two") == (w > 1 and w & (w - 1) == 0)
    assert all(any(abs(w - p) == 1 for p in F.ML_W_CLASSES["power_of_two"]) for w in F.ML_W_CLASSES["neighbour"])


def ml_windows_rightmost(values, valid, w, order):
    """`MM.windows` with the other tie rule: of equal smallest keys the RIGHTMOST."""
    whole, _ = MM.windows(values, valid, w, order)
    key = MM.keys_of(values, order)
    e = np.arange(values.size, dtype=np.int64)
    best, picked = key.copy(), e.copy()
    for j in range(1, w):             # from the right: only a strictly smaller key replaces the pick
        at = np.maximum(e - j, 0)
        take = key[at] < best
        best[take], picked[take] = key[at][take], at[take]
    return whole, picked


def ml_entries_from(values, strand, whole, picked, force_open=None, span_cap=None, strand_at_first_end=False):
    """`MM.entries_of` from the planes on: an entry opens where a whole window does not continue the pick of a whole window before it
    (or where `force_open` says so); its span runs to the next end that does not continue it (`span_cap(e)`: at most that)."""
    n = values.size
    before_whole = np.concatenate([[False], whole[:-1]])
    before_pick = np.concatenate([[-1], picked[:-1]])
    opens = whole & ~(before_whole & (before_pick == picked))
    if force_open is not None:
        opens |= whole & force_open
    e = np.flatnonzero(opens)
    stop = np.append(np.flatnonzero(~(whole & ~opens)), n)
    span = stop[np.searchsorted(stop, e, side="right")] - e
    if span_cap is not None:
        span = np.minimum(span, span_cap(e))
    a = picked[e]
    return MM.Entries(e, a, values[a], strand[e] if strand_at_first_end else strand[a], span)


def ml_wrong_rules(c, values, valid, strand):
    """name -> the entries a kernel with that defect would hold (the planted wrong rules)."""
    k, w, order = c.k, c.extra["w"], c.extra["order"]
    T = F.ML_TILE
    whole, picked = MM.windows(values, valid, w, order)
    e = np.arange(values.size, dtype=np.int64)
    out = {}
    out["rightmost on ties"] = ml_entries_from(values, strand, *ml_windows_rightmost(values, valid, w, order))
    # every tile its own batch: a window whose first end lies in the tile before is not whole (nothing in front of a tile is read)
    out["no halo"] = ml_entries_from(values, strand, whole & (e - (w - 1) >= e // T * T), picked)
    out["an entry opens at every tile start"] = ml_entries_from(values, strand, whole, picked, force_open=e % T == 0)
    out["span cut at the tile end"] = ml_entries_from(values, strand, whole, picked, span_cap=lambda x: (x // T + 1) * T - x)
    out["the order swapped"] = ml_entries_from(values, strand, *MM.windows(values, valid, w, MM.HASH if order == MM.LEX else MM.LEX))
    out["the strand of the first window end"] = ml_entries_from(values, strand, whole, picked, strand_at_first_end=True)
    return out


ML_WRONG = ("rightmost on ties", "no halo", "an entry opens at every tile start", "span cut at the tile end", "the order swapped",
            "the strand of the first window end")


def _same_csr(a, b):
    return all(np.asarray(x).shape == np.asarray(y).shape and np.array_equal(np.asarray(x).astype(np.uint64), np.asarray(y).astype(np.uint64))
               for x, y in zip(a, b))


def ml_case_report(rng, c) -> dict:
    """What one case of the stage contributes to the slice's conditions."""
    k, w, order, T = c.k, c.extra["w"], c.extra["order"], F.ML_TILE
    buf, off = c.buf(), c.offsets()
    values, valid, strand = MM.planes(buf, k, c.path, c.pre)
    whole, picked = MM.windows(values, valid, w, order)
    ent = MM.entries_of(buf, k, w, c.path, c.pre, order)
    true = MM.csr(ent, off, len(buf), k)
    assert _same_csr(true, MM.csr(ml_entries_from(values, strand, whole, picked), off, len(buf), k))   # the variants' frame is the model's
    assert _same_csr(true, F.ml_want(c, False))
    last = ent.end + ent.span.astype(np.int64) - 1
    # boundaries B = j * T with an entry whose windows [e, e + span) end on both sides of it: e < B <= e + span - 1
    straddled = {int(b) for b in (last // T * T)[(ent.end // T) < (last // T)]}
    # a window with two or more equal smallest keys whose leftmost lies in the tile before the window's end
    _, right = ml_windows_rightmost(values, valid, w, order)
    x = np.flatnonzero(whole & (right != picked))
    ties_across = int((picked[x] // T < x // T).sum())
    # records without a window; records whose run of whole windows is cut, told apart by the byte that cuts it: a junk byte of
    # `junk_bytes(pre)` that is no N (without the quality stream), or a base that the quality stream masks (with it)
    starts, ends = off[:-1].astype(np.int64), off[1:].astype(np.int64)
    n_whole = np.searchsorted(np.flatnonzero(whole), ends) - np.searchsorted(np.flatnonzero(whole), starts)
    a = np.frombuffer(buf, dtype=np.uint8)
    junk = np.setdiff1d(F.junk_bytes(c.pre), np.frombuffer(b"Nn", dtype=np.uint8))
    cut_junk = len({int(r) for r, p in ml_cuts(whole, off) if a[p] in junk})
    qs = c.qual_stream()
    whole_q, _ = MM.windows(*MM.planes(buf, k, c.path, c.pre, qs, c.cutoff)[:2], w, order)
    bases = np.frombuffer(b"ACGTacgt" + (b"Uu" if c.pre >= MM.PRE_NORMALIZE else b""), dtype=np.uint8)
    cut_masked = len({int(r) for r, p in ml_cuts(whole_q, off) if c.cutoff and a[p] in bases and qs[p] < c.cutoff})
    # the picked k-mer's start and the first window end lie in the same record: a whole window holds no break byte
    rec_of = lambda p: np.searchsorted(starts, p, side="right")   # noqa: E731
    same_record = bool(np.array_equal(rec_of(ent.picked - (k - 1)), rec_of(ent.end)))
    wrong = {name: not _same_csr(true, MM.csr(bad, off, len(buf), k)) for name, bad in ml_wrong_rules(c, values, valid, strand).items()}
    d = F.draw_ml(_copy(rng), c)
    second = F.ml_second_case(_copy_after(rng, c), c, d)
    return dict(order=order, path_pre=(c.path, c.pre), w=w, masked=not _same_csr(true, F.ml_want(c, True)), straddled=len(straddled),
                ties_across=ties_across, span1=int((ent.span == 1).sum()), span_w=int(((ent.span == w) & (w > 1)).sum()),
                span_mid=int(((ent.span > 1) & (ent.span < w)).sum()), no_window=int((n_whole == 0).sum()), cut_junk=cut_junk, cut_masked=cut_masked, same_record=same_record,
                wrong=wrong, prefix=d["prefix"], n_records=len(c.records), second_smaller=len(second.buf()) < len(buf),
                second_entries=len(F.ml_entries(second, d["second_q"])[0]), entries=len(ent))


def ml_cuts(whole, off):
    """(record, p) where a record's run of whole windows is cut: the window that ends at p - 1 is whole, the one that ends at p is not -
    so byte p is no base - and a later window of the same record is whole again."""
    ends = np.flatnonzero(whole)
    rec = np.searchsorted(off.astype(np.int64), ends, side="right") - 1
    gap = np.flatnonzero((np.diff(ends) > 1) & (rec[1:] == rec[:-1]))
    return [(rec[i], ends[i] + 1) for i in gap]


def _copy_after(rng, c):
    """A generator in the state the checker's is in after `draw_ml`."""
    g = _copy(rng)
    F.draw_ml(g, c)
    return g


def ml_slice_report(reports) -> dict:
    reports = list(reports)
    pow2 = lambda w: w & (w - 1) == 0   # noqa: E731
    cls = lambda w: next(name for name, ws in F.ML_W_CLASSES.items() if w in ws)   # noqa: E731
    return dict(orders={r["order"] for r in reports}, path_pres={r["path_pre"] for r in reports}, w_classes={cls(r["w"]) for r in reports},
                masked=sum(r["masked"] for r in reports), straddled=sum(r["straddled"] for r in reports),
                straddled_hash=sum(r["straddled"] for r in reports if r["order"] == MM.HASH),
                straddled_not_pow2=sum(r["straddled"] for r in reports if not pow2(r["w"])),
                ties_across=sum(r["ties_across"] for r in reports), span1=sum(r["span1"] for r in reports),
                span_w=sum(r["span_w"] for r in reports), span_mid=sum(r["span_mid"] for r in reports),
                no_window=sum(r["no_window"] for r in reports), cut_junk=sum(r["cut_junk"] for r in reports),
                cut_masked=sum(r["cut_masked"] for r in reports),
                same_record=all(r["same_record"] for r in reports),
                wrong={name: sum(r["wrong"][name] for r in reports) for name in ML_WRONG},
                second=all(r["second_smaller"] for r in reports) and sum(r["second_entries"] > 0 for r in reports),
                prefix=sum(r["prefix"] < r["n_records"] for r in reports))


def ml_conditions(r) -> list:
    """The conditions of the slice that do not hold (none: the slice means something)."""
    miss = []
    if r["orders"] != set(F.ML_ORDERS):
        miss.append("both orders")
    if r["path_pres"] != set(F.PATH_PRES):
        miss.append("every (path, pre) pair")
    if r["w_classes"] != set(F.ML_W_CLASSES):
        miss.append("all four classes of w")
    if r["masked"] < 1:
        miss.append("a quality mask that changes the CSR")
    if r["straddled"] < 8 or r["straddled_hash"] < 2 or r["straddled_not_pow2"] < 2:
        miss.append("8 straddled tile boundaries, 2 under HASH, 2 with w not a power of two")
    if r["ties_across"] < 1:
        miss.append("a tie whose leftmost pick lies across a tile boundary")
    if min(r["span1"], r["span_w"], r["span_mid"]) < 1:
        miss.append("spans 1, w and between")
    if r["no_window"] < 1 or r["cut_junk"] < 1 or r["cut_masked"] < 1:
        miss.append("a record without a window, one whose run of windows is cut by a junk byte and one where a masked base cuts it")
    miss += [f"wrong rule: {name}" for name, n in r["wrong"].items() if n < 1]
    if not r["second"] or r["prefix"] < 1:
        miss.append("a smaller second case with entries, a proper prefix")
    return miss


def test_minimizer_list_slice_meets_the_tile_boundaries_and_sees_every_planted_wrong_rule():
    reports = [ml_case_report(rng, c) for rng, c in cases("minimizer_list")]
    r = ml_slice_report(reports)
    assert ml_conditions(r) == [], r
    # `pos` relative to the record of the picked k-mer's start instead of the record of the first window end is no variant: with the
    # packer's offsets the two never differ.  A whole window is w + k - 1 good bases that end at the first window end, the picked k-mer
    # lies inside them, and every record ends with a break byte, which is no base: no record start lies between the two.
    assert r["same_record"]
    assert set(r["wrong"]) == set(ML_WRONG)


PINNED_NEWER = {"minimizer_list": ("915c437abf63380e3c45f19a0ee185a03e723827a6d22404ef024e7ebec1e5fd", (101, 15))}


def test_the_minimizer_list_slice_is_pinned():
    digest, size = PINNED_NEWER["minimizer_list"]
    assert F.SLICES["minimizer_list"] == size and F.slice_digest("minimizer_list") == digest


# ---- the map_reads stage ------------------------------------------------------------------------------------------------------------------
#
# Everything below is computed from `_lib_fuzz.pipeline_want` and `thinned_want` - the four host models on the case's bytes - by
# tests/_map_reads_report.py: no GPU.

import _align_model as AL  # noqa: E402
import _chain_model as CH  # noqa: E402
import _map_reads_report as R  # noqa: E402
import _mapping_model as MP  # noqa: E402
import _seed_index_model as SI  # noqa: E402


@functools.lru_cache(maxsize=None)
def map_reads_reports():
    """The report of every case of the slice.  A planted wrong rule that an earlier case has caught is not computed again (one case is
    what the condition asks for); the excused ones are computed on every case."""
    caught, out = set(), []
    excused = {(model, rule) for model, rule, _, _ in R.EXCUSED}
    for _, c in cases("map_reads"):
        out.append(R.case_report(c, skip=frozenset(caught)))
        caught |= {key for key, hit in out[-1]["mutants"].items() if hit and key not in excused}
    return tuple(out), frozenset(caught)


def test_the_map_reads_stage_draws_what_it_says():
    assert F.STAGES[-1] == "map_reads" and len(F.STAGES) == 13 and F.MAP_KS == (11, 15, 16, 17, 21)
    assert set(F.MAP_PRES) == {pre for path, pre in F.PATH_PRES if path == F.BITS_CANON} and len(F.MAP_PRES) == 4
    assert MP.LDS_CHAINS == 512 and CH.RING == 512 and AL.SEG_MAX == 4095
    kinds, classes, ws, orders, pres, n_refs = set(), set(), set(), set(), set(), set()
    drawn = {name: set() for name in F.MAP_CALL}
    for _, c in cases("map_reads"):
        e = c.extra
        cp, mp, ap = F.map_params(c)
        assert CH.check_params(cp) == CH.OK and MP.check_params(mp) == MP.OK and AL.check_params(ap) == AL.OK
        assert e["h"] in (1, 2, 63, 64, 65, 512) and e["best_n"] in (0, 1, 5) and e["band_pad"] in (0, 1, 16, 64)
        assert e["max_occ"] in (0, 1, 2, e["copies"] - 1, e["copies"]) and e["mask_level"] in (0.0, 0.5, 1.0) and e["pri_ratio"] in (0.0, 0.8, 1.0)
        assert set(F.map_kw(c)) == set(F.MAP_CALL) and 1 <= len(c.ref_records) <= 4 and 24 <= len(c.records) <= 64
        assert e["w"] in {w for ws_ in F.ML_W_CLASSES.values() for w in ws_}
        if e["cls"] == "repeat_family":
            assert e["max_dist"] <= 5 and e["min_cnt"] == 1 and e["min_score"] <= c.k and e["copies"] in F.MAP_FAMILY_COPIES
        lengths = {len(r) for r, kind in zip(c.records, c.kinds) if kind == "edge"}
        assert lengths == {0, 1, c.k - 1, c.k, c.k + e["w"] - 2, c.k + e["w"] - 1, c.k + e["w"]}
        assert not any(set(F.DELETED[c.pre]) & set(r) for r in c.records + c.ref_records)   # the excluded byte class
        assert max(len(r) for r in c.records) <= 1600
        kinds |= set(c.kinds)
        classes.add(e["cls"]); ws.add(e["w"]); orders.add(e["order"]); pres.add(c.pre); n_refs.add(len(c.ref_records))
        for name in F.MAP_CALL:
            drawn[name].add(e[name])
        assert 1 <= F.draw_map(_copy(cases("map_reads")[0][0]), c)["prefix"] < len(c.records)
    assert kinds >= {"cut", "unique", "long", "divergent", "long_indel", "bw_indel", "spacer", "chimera", "foreign", "head", "tail", "edge",
                     "family", "tandem", "family_x2", "dup"}, kinds
    assert classes == {"plain", "repeat_family"} and orders == set(F.ML_ORDERS) and len(pres) >= 2 and len(n_refs) >= 2 and len(ws) >= 3
    # each end of the two fractions and the default; the window at 1, 2 and CH_RING and on both sides of the 64-lane strip's edge
    # (64, 65; five cases do not also draw 63: the budgeted runs of tools/lib_fuzz.py do)
    assert 0 in drawn["q"] and {0.0, 0.5, 1.0} <= drawn["mask_level"] and {0.0, 0.8, 1.0} <= drawn["pri_ratio"], drawn
    assert {1, 2, 64, 65, 512} <= drawn["h"], drawn
    assert F.draw_extra(F.case_rng(F.SLICES["map_reads"][0], "map_reads", 1), "map_reads", 16)["cls"] in ("plain", "repeat_family")


def test_map_reads_slice_meets_its_conditions_and_sees_every_planted_wrong_rule():
    """Seeds, chains, mappings and alignments each on both sides of their rules; every CIGAR walked independently of the alignment
    model (`walk_cigars` asserts as it goes); the reads of known origin on their origin; every MUTANTS rule of the four models caught by
    at least one case, and each excused one by none."""
    reports, caught = map_reads_reports()
    r = R.slice_report(reports)
    assert R.conditions(r) == [], r
    every = set(R.all_mutants())
    excused = {(model, rule) for model, rule, _, _ in R.EXCUSED}
    assert len(every) == len(SI.MUTANTS) + len(CH.MUTANTS) + len(MP.MUTANTS) + len(AL.MUTANTS) == 27
    assert caught == every - excused and excused < every
    for model, rule, why, owner in R.EXCUSED:   # an excused rule changes no case of the slice, and a test elsewhere owns it
        assert r["mutants"][model, rule] == 0 and why and owner
        assert all((model, rule) in rep["mutants"] for rep in reports)


def test_two_cases_of_the_map_reads_slice_share_a_mapper():
    """The checker keeps one ReadMapper per (k, w, order): handle reuse is only exercised where two cases of the slice have one key.  At
    least one pair does, and its later case leaves some array of the handles larger and some smaller than the earlier case did."""
    sizes, seen, pairs = {}, {}, []
    for it, (_, c) in enumerate(cases("map_reads"), 1):
        p = F.pipeline_want(c)
        key = (c.k, c.extra["w"], c.extra["order"])
        sizes[it] = (len(c.records), int(p.read_list[1].size), p.n_anchors, p.chains.chain_rows.shape[0], p.chains.members.size, p.marks.out.size,
                     p.aln.cigar.size)
        if key in seen:
            pairs.append((seen[key], it))
        seen[key] = it
    assert pairs, seen
    assert any(any(b > a for a, b in zip(sizes[i], sizes[j])) and any(b < a for a, b in zip(sizes[i], sizes[j])) for i, j in pairs), (pairs, sizes)


def test_the_thinned_chains_keep_the_ends_and_the_order():
    for _, c in cases("map_reads"):
        p = F.pipeline_want(c)
        inp, sizes, want, chains = F.thinned_want(c)
        ap = F.map_params(c)[2]
        plain, plain_chains = AL.run(inp, ap)   # the shortcut of `_thinned_run` is the model's plain run
        assert all(np.array_equal(x, y) and x.dtype == y.dtype for x, y in zip(want, plain)) and AL.stats(inp, ap, want, chains) == AL.stats(inp, ap, plain, plain_chains)
        assert AL.verify(inp, ap) == AL.OK and inp.sel.size == p.marks.out.size == len(sizes)
        for s, (c0, size) in enumerate(zip(p.marks.out.tolist(), sizes)):
            full, thin = AL.members_of(p.inp.chains, c0), AL.members_of(inp.chains, s)
            assert thin[0] == full[0] and thin[-1] == full[-1] and [m for m in full if m in set(thin)] == thin
            assert (len(thin) < len(full)) == (size is not None)
            if size is not None:   # exactly one between part of the size searched for, at most max_seg: it is aligned
                parts = [(part[3], part[4]) for part in AL.parts_of(inp, s, ap) if part[0] == "between"]
                assert size in parts and max(size) <= ap.max_seg and (not chains[s].too_long or p.aligned[s].too_long)


PINNED_PIPELINE = {"map_reads": ("1d15849482701c59b551e96212312c84e47070a0445374784e853a9febcdb977", (123, 5))}


def test_the_map_reads_slice_is_pinned_and_the_twelve_before_it_did_not_move():
    digest, size = PINNED_PIPELINE["map_reads"]
    assert F.SLICES["map_reads"] == size and F.slice_digest("map_reads") == digest
    assert F.STAGES[:12] == F.OLD_STAGES + F.NEW_STAGES and {**PINNED_SLICES, "minimizer_list": (101, 15)}.items() <= F.SLICES.items()
    assert F.slice_digest("minimizer_list") == PINNED_NEWER["minimizer_list"][0]
    rng = F.case_rng(1, "minimizer_list", 1)
    assert rng.bit_generator.state == np.random.default_rng([1, 11, 1]).bit_generator.state   # a stage's index seeds its cases
