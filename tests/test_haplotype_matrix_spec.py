"""The haplotype-matrix spec (tests/spec_haplotype_matrix.py) on its own, without a GPU: the named cases, the spec against
the allele-frequency spec on the same GT columns, the bit planes against a NumPy packbits restatement, and the pieces of
the host layer that need no device."""
import numpy as np
import pytest

import spec_haplotype_matrix as spec
import spec_vcf_allele_frequencies as af_spec
from haplotype_matrix_cases import ERROR_CASES, GOOD_CASES, GUARD_TEXT, header_of
from vcf_af_cases import GOOD_CASES as AF_CASES, gt_line, text_of


def test_known_rows():
    text = text_of([gt_line([b"0|1", b"1/1", b"."]), gt_line([b"2|0", b"1", b".|10:7"]), gt_line([b"0|0", b"0|1", b"1|1"])],
                   header=header_of(3))
    codes, phased, n_samples, names = spec.haplotype_matrix(text)
    assert codes.tolist() == [[0, 1, 1, 1, 3, 3], [2, 0, 1, 3, 3, 2], [0, 0, 0, 1, 1, 1]]
    assert phased.tolist() == [0, 1, 1] and n_samples == 3 and names == ["S0", "S1", "S2"]
    codes, _, _, _ = spec.haplotype_matrix(text, ploidy=3)
    assert codes[1].tolist() == [2, 0, 3, 1, 3, 3, 3, 2, 3]
    ref_bits, alt_bits = spec.planes(spec.haplotype_matrix(text)[0])
    assert ref_bits[:, 0].tolist() == [0b101, 0b110, 0b100, 0, 0, 0] and alt_bits[:, 0].tolist() == [0, 1, 0b011, 0b101, 0b100, 0b100]


@pytest.mark.parametrize("name", sorted(GOOD_CASES))
def test_good_case_shapes_and_the_allele_frequency_spec(name):
    c = GOOD_CASES[name]
    codes, phased, n_samples, names = spec.haplotype_matrix(**c)
    lines = spec.data_lines(c["text"])
    assert codes.shape == (len(lines), n_samples * c["ploidy"]) and codes.dtype == np.uint8 and codes.max(initial=0) <= 3
    assert phased.shape == (len(lines),) and set(phased.tolist()) <= {0, 1}
    assert names is None or len(names) == n_samples
    want = af_spec.allele_frequencies(c["text"], "genotypes")
    for got, w in zip(spec.frequencies_of(codes, lines), want):
        assert np.array_equal(got.view(np.uint64), w.view(np.uint64))


@pytest.mark.parametrize("name", sorted(AF_CASES["genotypes"]))
def test_allele_frequency_cases_line_by_line(name):
    """Every line of the allele-frequency pass's own cases as a matrix of its own sample count, at a ploidy no GT exceeds."""
    for v, fields in enumerate(spec.data_lines(AF_CASES["genotypes"][name])):
        out = spec.line_row(fields, max(len(fields) - 9, 0), 8)
        if isinstance(out, int):                          # the only GTs of more than eight alleles in those cases
            assert out == 5 and any(g.count(b"/") > 7 for g in fields[9:])
            continue
        codes = np.array(out[0], dtype=np.uint8).reshape(1, -1)
        want = af_spec.genotype_line(fields, v)
        got = spec.frequencies_of(codes, [fields])
        assert (np.float64(got[0][0]).tobytes(), np.float64(got[1][0]).tobytes()) == \
            (np.float64(want[0]).tobytes(), np.float64(want[1]).tobytes())


@pytest.mark.parametrize("name", sorted(ERROR_CASES))
def test_error_case_names_the_lowest_line_and_kind(name):
    c, line, kind = ERROR_CASES[name]
    with pytest.raises(spec.HmError) as e:
        spec.haplotype_matrix(**c)
    assert (e.value.line, e.value.kind) == (line, kind)
    codes, phased, _, _, faults = spec.matrix_with_faults(**c)
    for v, _ in faults:
        assert np.all(codes[v] == 3) and phased[v] == 0


def test_guard_text_has_every_kind_of_line():
    codes, phased, n_samples, _, faults = spec.matrix_with_faults(GUARD_TEXT)
    assert n_samples == 2 and faults == [(1, 4), (3, 4), (4, 5), (5, 3)] and codes[0].tolist() == [0, 1, 1, 1]


def test_where_s_comes_from():
    assert spec.samples_of(GOOD_CASES["s_from_the_header"]["text"]) == (3, ["S0", "S1", "S2"])
    assert spec.samples_of(GOOD_CASES["s_from_the_last_chrom_line"]["text"]) == (2, ["S0", "S1"])
    assert spec.samples_of(GOOD_CASES["s_from_the_first_data_line"]["text"]) == (4, None)
    assert spec.samples_of(GOOD_CASES["s_from_the_argument"]["text"], 2) == (2, None)
    assert spec.samples_of(GOOD_CASES["s_from_the_argument_with_names"]["text"], 2) == (2, ["S0", "S1"])
    assert spec.samples_of(GOOD_CASES["s_0_from_the_argument"]["text"], 0) == (0, None)
    assert spec.samples_of(GOOD_CASES["header_only"]["text"]) == (3, ["S0", "S1", "S2"])
    assert spec.samples_of(b"") == (0, None) and spec.samples_of(GOOD_CASES["mixed_file"]["text"])[0] == 37


@pytest.mark.parametrize("n_variants", [0, 1, 63, 64, 65, 129])
@pytest.mark.parametrize("n_slots", [0, 1, 5])
def test_planes_equal_packbits(n_variants, n_slots):
    rng = np.random.default_rng([n_variants, n_slots])
    codes = rng.integers(0, 4, size=(n_variants, n_slots)).astype(np.uint8)
    for got, want in zip(spec.planes(codes), spec.planes_by_packbits(codes)):
        assert got.dtype == np.uint64 and got.shape == (n_slots, (n_variants + 63) // 64) and np.array_equal(got, want)


def test_host_layer_without_a_device(tmp_path):
    from graph_kmer_index_amd import vcf_files
    from graph_kmer_index_amd.vcf_files import HaplotypeMatrix, HaplotypeMatrixError
    assert vcf_files.STRIP == spec.STRIP and vcf_files.MAX_PLOIDY == spec.MAX_PLOIDY
    codes, phased, n_samples, names = spec.haplotype_matrix(**GOOD_CASES["s_from_the_header"])
    m = HaplotypeMatrix(codes, phased, n_samples, 2, names)
    m.to_file(str(tmp_path / "m"))
    back = HaplotypeMatrix.from_file(str(tmp_path / "m"))
    assert np.array_equal(back.codes, codes) and np.array_equal(back.phased, phased) and back.sample_names == names
    assert (back.n_samples, back.ploidy, back.n_variants) == (3, 2, 1)
    empty = HaplotypeMatrix(np.zeros((0, 6), np.uint8), np.zeros(0, np.uint8), 3, 2)
    assert [p.shape for p in empty.planes()] == [(6, 0), (6, 0)]
    no_slots = HaplotypeMatrix(np.zeros(0, np.uint8), np.ones(4, np.uint8), 0, 2)
    assert no_slots.codes.shape == (4, 0) and [p.shape for p in no_slots.planes()] == [(0, 1), (0, 1)]
    assert HaplotypeMatrix(np.zeros(0, np.uint8), np.zeros(0, np.uint8), 0, 2).codes.shape == (0, 0)
    for bad in (lambda: HaplotypeMatrix(codes, phased, n_samples, 2, ["one"]), lambda: HaplotypeMatrix(codes, phased, 2, 2)):
        with pytest.raises(ValueError):
            bad()
    e = HaplotypeMatrixError(7, 4, 3, 2)
    assert isinstance(e, ValueError) and (e.line, e.kind) == (7, 4) and "data line 7:" in str(e)
