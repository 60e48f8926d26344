"""The kernels the library ships equal the builds its dispatch can reach (tests/_builds.py), and every other kernel names the test that runs it.

The shipped code object is read with ROCm's LLVM tools (the .hip_fatbin section, one offload bundle per object file, the gfx950 code
object of each, its `.kd` symbols).  No GPU: this runs in seconds on the library the suite builds."""
import os
import re

import pytest

import _builds as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "needletail_amd", "libneedletail_amd.so")

# every kernel outside the dispatch matrix, with the test that launches it (file, test function)
OTHER_KERNELS = {
    "fold_kernel": ("test_gpu_build_matrix.py", "test_reduce_entries_against_the_oracle"),
    "synth_reads_kernel": ("test_gpu_parity.py", "test_device_synth_matches_cpu_generator"),
    "revcomp_records_kernel": ("test_gpu_parity.py", "test_full_size_properties_config2"),
    "map_reverse_kernel": ("test_gpu_parity.py", "test_normalize_strip_revcomp_random"),
    "compact_count_kernel": ("test_gpu_parity.py", "test_normalize_strip_revcomp_random"),
    "compact_scan_kernel": ("test_gpu_parity.py", "test_normalize_strip_revcomp_random"),
    "compact_write_kernel": ("test_gpu_parity.py", "test_normalize_strip_revcomp_random"),
    "quality_mask_kernel": ("test_gpu_parity.py", "test_minimizer_and_quality_mask_kats"),
    "bit_minimizer_kernel": ("test_gpu_parity.py", "test_minimizer_and_quality_mask_kats"),
    "minimizer_bytes_kernel": ("test_gpu_parity.py", "test_minimizer_and_quality_mask_kats"),
    "minimizer_emit_kernel": ("test_gpu_parity.py", "test_minimizer_and_quality_mask_kats"),
    "bit_canonical_kernel": ("test_gpu_parity.py", "test_bit_reverse_complement_and_canonical_kats"),
    "canonical_bytes_kernel": ("test_gpu_parity.py", "test_batched_compat_face_matches_the_iterators_per_record"),
    "pack_flags8_kernel": ("test_gpu_parity.py", "test_batched_compat_face_matches_the_iterators_per_record"),
    "cp_count_kernel": ("test_gpu_parity.py", "test_batched_compat_face_matches_the_iterators_per_record"),
    "cp_scan_kernel": ("test_gpu_parity.py", "test_batched_compat_face_matches_the_iterators_per_record"),
    "cp_scatter_kernel": ("test_gpu_parity.py", "test_batched_compat_face_matches_the_iterators_per_record"),
    "mark_record_starts_kernel": ("test_gpu_parity.py", "test_bit_kmers_planes_face_matches_the_iterator_per_record"),
    "bit_kmers_planes_kernel<true>": ("test_gpu_parity.py", "test_bit_kmers_planes_face_matches_the_iterator_per_record"),
    "bit_kmers_planes_kernel<false>": ("test_gpu_parity.py", "test_bit_kmers_planes_face_matches_the_iterator_per_record"),
    "canonical_bytes_planes_kernel": ("test_gpu_parity.py", "test_batched_compat_face_matches_the_iterators_per_record"),
    "minimizer_batch_kernel": ("test_gpu_parity.py", "test_minimizer_batch_matches_the_reference_function_per_record"),
    "minimizer_emit_record_kernel": ("test_gpu_parity.py", "test_minimizer_batch_matches_the_reference_function_per_record"),
    "(anonymous namespace)::xor_from_bit_counters_kernel": ("test_gpu_parity.py", "test_rccl_allreduce_through_the_c_abi_single_rank"),
}


def check(library: set, manifest: set, other: dict):
    """The list of problems (empty: the library and the manifest agree)."""
    problems = []
    matrix = {s for s in library if B.family(s) in B.MATRIX_FAMILIES}
    problems += [f"shipped build no call reaches: {s}" for s in sorted(matrix - manifest)]
    problems += [f"manifest build not in the library: {s}" for s in sorted(manifest - matrix)]
    problems += [f"kernel neither in the matrix nor in OTHER_KERNELS: {s}" for s in sorted(library - matrix - set(other))]
    problems += [f"OTHER_KERNELS entry not in the library: {s}" for s in sorted(set(other) - library)]
    return problems


@pytest.fixture(scope="module")
def library():
    return B.library_kernels(SO)


@pytest.fixture(scope="module")
def manifest():
    return B.manifest()


def test_the_library_holds_exactly_the_reachable_builds(library, manifest):
    assert check(library, set(manifest), OTHER_KERNELS) == []


def test_every_other_kernel_names_an_existing_test():
    for sym, (fname, test) in OTHER_KERNELS.items():
        src = open(os.path.join(ROOT, "tests", fname)).read()
        assert re.search(rf"^def {re.escape(test)}\(", src, re.M), (sym, fname, test)


def test_the_manifest_counts(manifest):
    """The matrix by family.  No build with TIE_RC && !ACCEPT_U outside the k-mer reduce (the speculative scan2 builds of the byte path on
    input that was not normalised): minimizers and materialise mode reject that input."""
    fam = {}
    for s in manifest:
        fam[B.family(s)] = fam.get(B.family(s), 0) + 1
    assert fam == {"scan2_kernel": 32 * 4 + 32 * 2 + 32 * 6 + 9 * 5 * 3 + 2 * 3, "minimizer_scan_kernel": 8 * 6,
                   "scan_kernel": 2 * 5 * 2 + 3, "canonical_bytes_reduce_kernel": 4, "wide_canonical_reduce_kernel": 4,
                   "window_min_reduce_kernel": 16}
    spec = [s for s in manifest if re.match(r"(scan2_kernel<\d+|minimizer_scan_kernel<\d|scan_kernel<\d, true), true, false,", s)]
    assert all(c.entry == "reduce" and c.path == B.PATH_BYTES_CANONICAL and c.pre < B.PRE_NORMALIZE for s in spec for c in manifest[s])
    assert len(spec) == 64   # the speculative builds: 32 k, with and without a quality stream


def test_every_route_bit_selects_its_builds(manifest):
    """The route switches reach what they name: NO_F64 the non-f64 generic builds, NO_REGFUSED | NO_GENERIC the two-pass route, NO_SPECULATION
    the byte-walking kernel alone."""
    by_route = {}
    for s, cs in manifest.items():
        for c in cs:
            by_route.setdefault(c.route, set()).add(s)
    assert any(s.startswith("minimizer_scan_kernel") and ", false, 1>" in s for s in by_route[B.ROUTE_NO_F64])
    assert "window_min_reduce_kernel<7>" in by_route[B.ROUTE_NO_REGFUSED | B.ROUTE_NO_GENERIC]
    assert by_route[B.ROUTE_NO_SPECULATION] == {B.bytes_reduce(w, q) for w in (False, True) for q in (False, True)}
    assert B.kernels(B.Call("reduce", 21, 0, B.PATH_BYTES_CANONICAL, B.PRE_NONE, False, 0)) == (
        "scan2_kernel<21, true, false, false, 14, 0, false>", "canonical_bytes_reduce_kernel<false, false>")
    assert B.kernels(B.Call("minimizers", 21, 11, B.PATH_BYTES_CANONICAL, B.PRE_NONE, False, 0)) is None
    assert B.kernels(B.Call("materialize", 21, 0, B.PATH_BYTES_CANONICAL, B.PRE_STRIP_RETURNS, True, 0)) is None


def test_the_checker_sees_a_missing_build(library, manifest):
    """The check is not vacuous: a symbol taken out of the library, an unknown kernel added, a manifest entry added, all show."""
    victim = "scan2_kernel<19, false, true, true, 14, 0, true>"   # a forward-only quality build, k = 19
    assert victim in library
    assert check(library - {victim}, set(manifest), OTHER_KERNELS) == [f"manifest build not in the library: {victim}"]
    assert check(library | {"scan2_kernel<21, true, false, false, 14, 11, false>"}, set(manifest), OTHER_KERNELS) == [
        "shipped build no call reaches: scan2_kernel<21, true, false, false, 14, 11, false>"]
    assert check(library | {"new_kernel"}, set(manifest), OTHER_KERNELS) == ["kernel neither in the matrix nor in OTHER_KERNELS: new_kernel"]
    assert check(library, set(manifest) - {victim}, OTHER_KERNELS) == [f"shipped build no call reaches: {victim}"]


def test_short_names():
    assert B.short_name("void ntk::scan2_kernel<5, false, true, false, 14, 0, false>(ntk::ScanArgs) (.kd)") == \
        "scan2_kernel<5, false, true, false, 14, 0, false>"
    assert B.short_name("(anonymous namespace)::xor_from_bit_counters_kernel(unsigned long*) (.kd)") == \
        "(anonymous namespace)::xor_from_bit_counters_kernel"
    assert B.short_name("ntk::fold_kernel(unsigned int const*, unsigned long const*, int)") == "fold_kernel"
