"""The k-mer counter's semantics pinned against the reference itself (no GPU): KmerFrequencyIndex.from_kmers of the imported
reference equals the NumPy restatement, and the reference's consumers of a frequency source -- run live with a dict-backed
counter, whose get_frequency adds no reverse complement -- equal the test-side restatements under that rule and the
outputs recorded in tests/golden/kmer_counter_reference.json.gz."""
import logging
import os
import sys

import numpy as np
import pytest

import spec_kmer_counter as spec
import spec_structural_variants as spec_sv
import uvk_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SV = {c["name"]: c for c in spec_sv.load_cases()}
UVK = {c["name"]: c for c in uvk_golden.load_cases()}


@pytest.fixture(scope="module")
def driver():
    """tests/golden/make_golden_kmer_counter.py: the functions that run the reference on a stored case."""
    saved = list(sys.path)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    logging.disable(logging.CRITICAL)
    try:
        import make_golden_kmer_counter
        yield make_golden_kmer_counter
    finally:
        logging.disable(logging.NOTSET)
        sys.path[:] = saved


def _same(got, exp, what):
    for name, a, b in zip(("hashes", "nodes", "ref_offsets", "allele_frequencies"), got, exp):
        assert len(a) == len(b) and np.array_equal(np.asarray(a).astype(np.float64), np.asarray(b).astype(np.float64)), \
            (what, name)


# ------------------------------------------------------------------ restatements against the recorded outputs (always run)
@pytest.mark.parametrize("name", spec.SV_CASES)
def test_sv_spec_without_reverse_complement_equals_recorded_reference(name):
    _same(spec.sv_expected_no_rc(SV[name]), spec.flat_columns(spec.golden()["sv"][name]), name)


@pytest.mark.parametrize("name", spec.UVK_CASES)
def test_uvk_spec_without_reverse_complement_equals_recorded_reference(name):
    _same(spec.uvk_expected_no_rc(UVK[name]), spec.flat_columns(spec.golden()["uvk"][name]), name)


def test_frequency_index_spec_equals_recorded_reference():
    rec = spec.golden()["frequency_index"]
    for name, kmers in spec.frequency_index_inputs().items():
        u, c = spec.unique_counts(kmers)
        assert (str(u.dtype), str(c.dtype)) == (rec[name]["dtypes"]["kmers"], rec[name]["dtypes"]["frequencies"]), name
        assert u.tolist() == rec[name]["kmers"] and c.tolist() == rec[name]["frequencies"], name


def test_a_recorded_case_separates_the_two_rules():
    """max_frequency_2 holds windows whose own count is 0 while their reverse complement's is >= max_frequency, and the
    recorded output with the counter differs from the one recorded with the index."""
    case = SV["max_frequency_2"]
    t = spec_sv.case_table(case)
    g = spec_sv.case_graph(case)
    n = 0
    for node in np.asarray(case["pairs"]).reshape(-1).tolist():
        if g.get_node_size(node) > case["k"] + 5:
            h = spec_sv.window_hashes(g.get_numeric_node_sequence(node), case["k"])
            n += int(((t.first_hit(h) == 0) & (t.first_hit(spec_sv.revcomp(h, 31)) >= case["max_frequency"])).sum())
    assert n > 0
    with_counter = spec.flat_columns(spec.golden()["sv"]["max_frequency_2"])[0]
    assert with_counter.tolist() != spec_sv.expected(case)[0].tolist()


# ------------------------------------------------------------------ the live reference
@pytest.mark.reference
def test_reference_frequency_index_equals_spec(driver):
    rng = np.random.default_rng(5)
    inputs = dict(spec.frequency_index_inputs())
    inputs["random_small_range"] = rng.integers(0, 1000, size=20000, dtype=np.uint64)
    rec = spec.golden()["frequency_index"]
    for name, kmers in inputs.items():
        got = driver.reference_frequency_index(kmers)
        u, c = spec.unique_counts(kmers)
        assert got["kmers"] == u.tolist() and got["frequencies"] == c.tolist(), name
        assert got["dtypes"] == {"kmers": "uint64", "frequencies": "int64"}, name
        if name in rec:
            assert got == rec[name], name


@pytest.mark.reference
@pytest.mark.parametrize("name", spec.SV_CASES)
def test_reference_sv_with_a_counter_equals_spec_and_golden(driver, name):
    got = driver.columns(driver.reference_sv(SV[name]))
    assert got == spec.golden()["sv"][name]
    _same(spec.flat_columns(got), spec.sv_expected_no_rc(SV[name]), name)


@pytest.mark.reference
@pytest.mark.parametrize("name", spec.UVK_CASES[:2])
def test_reference_uvk_with_a_counter_equals_spec_and_golden(driver, name):
    got = driver.columns(driver.reference_uvk(UVK[name]))
    assert got == spec.golden()["uvk"][name]
    _same(spec.flat_columns(got), spec.uvk_expected_no_rc(UVK[name]), name)
