"""The fixed slices of the structured differential fuzz of the sixteen libraries (tests/_lib_fuzz.py: the twelve k-mer libraries, and the
seed index, the chains, the mappings and the alignments as one pipeline) on a real MI355X: one test per stage and width, thirteen stages,
each a fixed seed and a fixed number of cases (`_lib_fuzz.SLICES`).  tests/test_lib_fuzz_inputs.py proves without a GPU
that every slice holds the content kinds, the edge lengths and the two-sided conditions that make it mean something; longer runs go
through tools/lib_fuzz.py and are recorded under profiles/lib_fuzz/.  Truth is the existing host models; every comparison is exact."""
import pytest

torch = pytest.importorskip("torch")

import needletail_amd as nt  # noqa: E402
import _lib_fuzz as F  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sess():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = nt.Context(0)
    s = F.Session(c)
    yield s
    s.close()
    c.close()


def test_sketch_and_count_narrow(sess):
    F.run_slice(sess, "count")


def test_sketch_and_count_wide(sess):
    F.run_slice(sess, "count_wide")


def test_minhash_stateful_narrow(sess):
    F.run_slice(sess, "minhash")


def test_minhash_stateful_wide(sess):
    F.run_slice(sess, "minhash_wide")


def test_abundance(sess):
    F.run_slice(sess, "abundance")


def test_trim_compact_and_round_trip(sess):
    F.run_slice(sess, "trim")


def test_record_minhash_and_the_set_behind_it(sess):
    F.run_slice(sess, "record_minhash")


def test_kmer_sets_narrow(sess):
    F.run_slice(sess, "kmer_sets")


def test_kmer_sets_wide(sess):
    F.run_slice(sess, "kmer_sets_wide")


def test_dbg_and_its_unitig_batch(sess):
    F.run_slice(sess, "dbg")


def test_colors_and_the_compacted_batch(sess):
    F.run_slice(sess, "colors")


def test_minimizer_list(sess):
    F.run_slice(sess, "minimizer_list")


def test_map_reads_pipeline(sess):
    """The thirteenth stage: references indexed and reads mapped and aligned on one ReadMapper per (k, w, order) that outlives its
    cases, every field and stats word of the four handles against the host models; a prefix on the same handles; thinned chains."""
    F.run_slice(sess, "map_reads")
