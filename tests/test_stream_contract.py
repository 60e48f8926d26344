"""tests/_stream_contract.py held to the headers: every device-face declaration has a row, every row's words stand in the header next to
its declaration (or in the head comment, which then names the call), every row names a GPU test that exists, and what the GPU tests rely on
in the sources is still their text."""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _libraries as L  # noqa: E402
import _stream_contract as SC  # noqa: E402

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(SC.ROOT, "needletail_amd", "csrc")


def declared():
    """function -> (header, parameter text, comment text next to it) over the thirteen headers."""
    out = {}
    for header in SC.HEADERS:
        for name, params, near in SC.declarations(SC.header_text(header)):
            assert name not in out, name
            out[name] = (header, params, near)
    return out


def test_the_thirteen_headers_are_the_ones_that_ship():
    """Every header below include/, whatever its directory: the twelve needletail_amd(_NAME).h and those of include/needletail_amd/."""
    shipped = SC.shipped_headers()
    assert all(re.fullmatch(r"needletail_amd(_\w+)?\.h|needletail_amd/\w+\.h", f) for f in shipped), shipped
    assert shipped == sorted(SC.HEADERS) and len(SC.HEADERS) == 13


def test_every_device_face_declaration_has_a_row():
    decl = declared()
    for name in SC.NAMED:
        assert name in decl and not SC.takes_device_pointer(decl[name][1]), name
    required = {name for name, (_, params, _) in decl.items() if SC.takes_device_pointer(params)} | set(SC.NAMED)
    rows = [r.function for r in SC.ROWS]
    assert len(set(rows)) == len(rows), "a call is listed twice"
    assert set(rows) == required, sorted(set(rows) ^ required)
    for r in SC.ROWS:
        assert decl[r.function][0] == r.header, r.function


def test_the_device_pointer_rule_sees_the_parameters_it_is_for():
    decl = declared()
    assert SC.takes_device_pointer(decl["ntk_reduce_device"][1]) and "uint8_t *d_seq" in decl["ntk_reduce_device"][1]
    assert SC.takes_device_pointer(decl["ntk_kmer_colors_add_device"][1])
    for host_only in ("ntk_canonical_kmers_batch", "ntk_minhash_compare", "ntk_mhset_add", "ntk_batch_append"):   # the compat face and host work
        assert not SC.takes_device_pointer(decl[host_only][1]), host_only


@pytest.mark.parametrize("row", SC.ROWS, ids=lambda r: r.function)
def test_a_rows_words_are_the_headers(row):
    assert row.cls in (SC.ASYNC, SC.MAY_SYNC, SC.SYNC) and row.where in ("decl", "head")
    text = SC.header_text(row.header)
    if row.where == "decl":
        near = {name: near for name, _, near in SC.declarations(text)}[row.function]
        assert SC.plain(row.words) in SC.plain(near), (row.function, "the words are not at the declaration")
    else:
        head = SC.plain(SC.head_comment(text))
        assert SC.plain(row.words) in head, (row.function, "the words are not in the head comment")
        # the head comment's sentence covers the call: it speaks of every call, or names this one's verb
        verb = row.function.replace("_device", "").rsplit("_", 1)[1]
        if row.header == SC.HEADERS[-1] and row.function.endswith("_device"):   # the minimizer list's sentence says "run_device"
            verb += "_device"
        assert "Every call" in row.words or re.search(rf"\b{verb}\b", row.words), (row.function, verb)
    # the class is what the words say
    said = SC.plain(row.words).lower()
    if row.cls == SC.ASYNC:
        assert re.search(r"async|queued on the stream|queues nothing", said), row.function
    elif row.cls == SC.MAY_SYNC:
        assert "may synchronise" in said, row.function
    else:
        assert re.search(r"synchronises|synchronise it|synchronous", said) and "may" not in said, row.function


def test_every_row_names_a_gpu_test_that_exists():
    texts = {f: open(os.path.join(TESTS, f)).read() for f in {r.file for r in SC.ROWS}}
    assert SC.GPU_TESTS in texts and set(texts) == {SC.GPU_TESTS, "test_gpu_minimizer_list.py"}
    assert all(r.file == SC.GPU_TESTS or r.function.startswith("ntk_minimizer_list_") for r in SC.ROWS)   # a row's own file is its library's
    for text in texts.values():
        assert re.search(r"^pytestmark = pytest\.mark\.gpu", text, re.M)
    for row in SC.ROWS:
        text = texts[row.file]
        m = re.search(rf"^def {re.escape(row.test)}\(.*?(?=^def |^class |\Z)", text, re.M | re.S)
        assert m, (row.function, row.test)
    # and the call is made in that file: by name through ctypes, or through the handle's entry or facade method of that name
    for row in SC.ROWS:
        text = texts[row.file]
        short = re.sub(r"^ntk_(kmer_table|wide_table|kmer_sketch|minhash|read_abundance|read_trim|record_minhash|mhset|kmer_sets|dbg|kmer_colors|minimizer_list)_", "", row.function)
        facade = {"ntk_reduce_device_quality": "reduce_device", "ntk_kmer_table_extract_device": "extract(", "ntk_wide_table_extract_device": "extract(",
                  "ntk_minhash_read": ".hashes()", "ntk_record_minhash_read": ".sketches", "ntk_mhset_read": ".sketch(", "ntk_batch_submit": ".submit(",
                  "ntk_kmer_table_stats": ".stats()", "ntk_wide_table_stats": ".stats()", "ntk_kmer_sketch_registers": ".registers()",
                  "ntk_kmer_sketch_estimate": ".estimate()", "ntk_record_minhash_stats": ".stats()", "ntk_record_minhash_trim": "rmh.trim",
                  "ntk_minimizer_list_result_device": ".device_arrays()", "ntk_minimizer_list_stats": ".stats()"}.get(row.function)
        names = [row.function, row.function.replace("ntk_", "", 1) + "(", f'"{short}"', f".{short}(", facade]
        assert any(n and n in text for n in names), (row.function, names)


def test_the_inventory_table_of_the_profile_is_this_one():
    readme = os.path.join(SC.ROOT, "profiles", "stream_order", "README.md")
    text = open(readme).read()   # the whole table: a blank line follows its last row, so rows taken off the end are missed too
    assert SC.table_markdown() + "\n\n" in text, "profiles/stream_order/README.md: regenerate the table from _stream_contract.table_markdown()"


def test_what_the_growth_cases_rely_on_in_the_sources():
    """The two growth cases of the GPU file take their sizes from these lines."""
    consumer = L.no_comments(open(os.path.join(CSRC, "ntk_consumer.hpp")).read())
    for array in ("d_values", "d_valid16", "d_rc16"):
        assert re.search(rf"{array}\.ensure\(stream, need(?: / 16)?, grow_exact\)", consumer), array
    mem = L.no_comments(open(os.path.join(CSRC, "ntk_device_mem.hpp")).read())
    assert "if (p) CT_HIPCHK(hipStreamSynchronize(stream));" in mem and "inline uint64_t grow_exact(uint64_t, uint64_t need) { return need; }" in mem
    api = L.no_comments(open(os.path.join(CSRC, "ntk_api.hip")).read())
    assert "c->d_part_hist.ensure(c->stream, (uint64_t)blocks * kHistBins, grow_exact)" in api
    plan = L.no_comments(open(os.path.join(CSRC, "ntk_plan.hpp")).read())
    assert "const uint64_t want_blocks = (tiles + chunk * waves_per_block - 1) / (chunk * waves_per_block);" in plan
    assert "uint64_t chunk = tiles / (blocks_max * waves_per_block * 4);" in plan
    tile = L.no_comments(open(os.path.join(CSRC, "ntk_tile.hpp")).read())
    assert "return km > 32 ? 61 * 16 : (!exact ? 62 * 16 : (km <= 16 ? 63 * 16 : ((kTileBytes - (km - 1)) & ~3)));" in tile
    import _stream_order as S
    stride, waves = (1024 - 20) & ~3, 12   # the k = 21 build; 768 threads a block (needletail_amd.h, ntk_ctx_set_launch)
    small, big = S.batches(21)[0].n, S.GROW_READS[2] * (S.GROW_READS[3] + 1)
    assert -(-small // stride) <= waves, "the small batch is one block's worth of tiles"
    assert -(-(-(-big // stride)) // waves) >= 2, "the large batch needs more partial rows"
