"""The VCF-file rules (tests/spec_vcf_parse.py) pinned without a GPU against their oracle, VariantArrays.from_vcf, on the
buffers of tests/vcf_cases.py; the host-side join of pieces (vcf_files.VariantPieces) at every cut; the C ABI's two
declarations and the command line's two flags."""
import os
import re

import numpy as np
import pytest

import spec_vcf_parse as spec
import vcf_cases as cases
from graph_kmer_index_amd import _lib, vcf_files
from graph_kmer_index_amd.unique_variant_kmers import VariantArrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_arrays(tmp_path, data, name="case.vcf"):
    path = str(tmp_path / name)
    with open(path, "wb") as fh:
        fh.write(data)
    return VariantArrays.from_vcf(path)


def assert_same_variants(got, want):
    assert got.positions.dtype == want.positions.dtype == np.int64 and np.array_equal(got.positions, want.positions)
    assert got.line_numbers.dtype == want.line_numbers.dtype == np.int64
    assert np.array_equal(got.line_numbers, want.line_numbers)
    assert got.is_snp.dtype == want.is_snp.dtype == np.int8 and np.array_equal(got.is_snp, want.is_snp)
    assert got.chromosomes.dtype == want.chromosomes.dtype == object and got.chromosomes.shape == want.chromosomes.shape
    assert got.chromosomes.tolist() == want.chromosomes.tolist()


def joined(pieces):
    """The pieces (bytes, each of whole lines) through the spec and the package's join."""
    out = vcf_files.VariantPieces()
    for p in pieces:
        arrays, bad = spec.piece(p)
        assert bad == (-1, 0)
        out.add(*arrays)
    return out


@pytest.mark.parametrize("name", sorted(cases.GOOD))
def test_spec_equals_from_vcf(name, tmp_path):
    data = cases.GOOD[name]
    out = joined([data])
    assert out.n_lines == len(spec.lines_of(data))
    assert_same_variants(out.variant_arrays(), host_arrays(tmp_path, data))


def test_the_listed_cases_are_there():
    g, T = cases.GOOD, cases.T
    assert [len(g[k]) for k in ("bytes_4095", "bytes_4096", "bytes_4097")] == [T - 1, T, T + 1]
    assert g["newline_at_4095"][T - 1:T] == b"\n" and g["newline_at_4096"][T:T + 1] == b"\n"
    assert g["tab_at_4096"][T:T + 1] == b"\t" and g["tab_at_4096"][:T].rfind(b"\t") < g["tab_at_4096"][:T].rfind(b"\n")
    assert max(len(x) for x in g["genotypes_over_a_tile"].split(b"\n")) > T
    assert max(len(x) for x in g["genotypes_over_64k"].split(b"\n")) > 65536
    assert spec.parse(g["field_counts"])["is_snp"].tolist() == [-1, -1, 1, 1, -1, 0]
    assert spec.parse(g["ref_alt_pairs"])["is_snp"].tolist() == [1, 0, 0, 0, 0, 0]
    assert spec.parse(g["pos_forms"])["positions"].tolist() == [7, 123456789012345678, 0, 0]
    assert spec.run_name_list(spec.parse(g["prefix_names"])) == ["1", "11", "1", "chr1", "chr10", "chr1"]
    assert spec.parse(g["prefix_names"])["chrom_run"].tolist() == [0, 0, 1, 1, 2, 3, 4, 4, 5, 5]
    assert spec.run_name_list(spec.parse(g["return_to_a_name"])) == ["1", "2", "1"]
    assert spec.run_name_list(spec.parse(g["empty_chrom"])) == ["", "1", ""]
    assert g["crlf"].count(b"\r\n") == g["crlf"].count(b"\n") and not g["open_end"].endswith(b"\n")
    assert spec.parse(b"")["run_name_start"].tolist() == [0] and spec.parse(cases.HEADER)["n_lines"] == 2
    assert set(cases.UNALIGNED) <= set(g)


@pytest.mark.parametrize("name", sorted(cases.BAD))
def test_bad_lines(name, tmp_path):
    data, line, kind = cases.BAD[name]
    out = spec.parse(data)
    assert (out["first_bad_variant"], out["first_bad_kind"]) == (line, kind)
    message = str(vcf_files.bad_line_error(line, kind))
    assert str(line) in message
    if kind == 1:                                       # the host route's own words
        with pytest.raises(ValueError) as e:
            host_arrays(tmp_path, data)
        assert str(e.value) == message == spec.KIND1_TEXT % line
    else:
        assert "POS" in message and "digits" in message


@pytest.mark.parametrize("name", sorted(n for n in cases.GOOD if len(cases.GOOD[n]) < 300))
def test_two_pieces_cut_at_every_byte_join_to_the_whole(name, tmp_path):
    """A cut at any byte, moved to the line end before it as iter_line_chunks cuts (a piece ends at a line end)."""
    data = cases.GOOD[name]
    want = host_arrays(tmp_path, data)
    cuts = sorted({data.rfind(b"\n", 0, at) + 1 for at in range(len(data) + 1)})
    assert len(data) in cuts or not data.endswith(b"\n")
    for cut in cuts:
        pieces = [p for p in (data[:cut], data[cut:]) if p]
        out = joined(pieces)
        assert out.n_lines == len(spec.lines_of(data)), cut
        assert_same_variants(out.variant_arrays(), want)


def test_pieces_of_one_line_each_join_runs():
    data = cases.GOOD["prefix_names"] + cases.GOOD["return_to_a_name"] + cases.HEADER + cases.GOOD["empty_chrom"]
    out = joined(data.splitlines(keepends=True))
    whole = spec.parse(data)
    assert out.run_names == spec.run_name_list(whole)
    assert np.array_equal(np.concatenate(out.run_of_variant), whole["chrom_run"])


def test_iter_line_chunks_pieces_join_to_the_whole(tmp_path):
    import io
    from graph_kmer_index_amd.read_files import iter_line_chunks
    data = cases.GOOD["many_lines"]
    want = host_arrays(tmp_path, data)
    for chunk_bytes in (64, 1000, 10 ** 6):
        assert_same_variants(joined(list(iter_line_chunks(io.BytesIO(data), chunk_bytes))).variant_arrays(), want)


def _arity(name):
    text = open(os.path.join(ROOT, "include", "gki.h")).read()
    m = re.search(r"\nint %s\(([^;]*)\);" % name, text)
    assert m, name
    return m.group(1).count(",") + 1


def test_the_symbols_are_declared_and_bound():
    assert _arity("gki_vcf_parse_count") == len(_lib.SYMBOLS["gki_vcf_parse_count"][1]) == 8
    assert _arity("gki_vcf_parse_emit") == len(_lib.SYMBOLS["gki_vcf_parse_emit"][1]) == 10
    assert "VCF files" in open(os.path.join(ROOT, "include", "gki.h")).read()


def test_cli_parser_has_the_flags():
    from graph_kmer_index_amd.command_line_interface import build_parser
    base = ["make_unique_variant_kmers", "-g", "g", "-V", "v", "-k", "31", "-o", "o"]
    a = build_parser().parse_args(base)
    assert (a.vcf_parse, a.inflate) == ("auto", "auto")
    a = build_parser().parse_args(base + ["--vcf-parse", "host", "--inflate", "device"])
    assert (a.vcf_parse, a.inflate) == ("host", "device")
    with pytest.raises(SystemExit):
        build_parser().parse_args(base + ["--vcf-parse", "gpu"])
    assert hasattr(VariantArrays, "from_vcf_on_device")
