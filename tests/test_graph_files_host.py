"""Host side of the graph build that needs no device: one read of the FASTA for every record, the error's text and
the command's arguments."""
import numpy as np
import pytest

from graph_kmer_index_amd.command_line_interface import build_parser, make_graph
from graph_kmer_index_amd.graph_files import GraphBuildError
from graph_kmer_index_amd.snp_kmer_finder import read_fasta_record, read_fasta_records


def test_records_come_from_one_read_in_file_or_chosen_order(tmp_path):
    path = str(tmp_path / "ref.fa")
    with open(path, "wb") as f:
        f.write(b">chr2 a description\nACGT\r\nAC\n>chr1\nGG\n>\nT\n>chr1 again\nTTTT")
    names, records = read_fasta_records(path)
    assert names == ["chr2", "chr1", "", "chr1"]
    assert [r.tobytes() for r in records] == [b"ACGTAC", b"GG", b"T", b"GG"]      # a name twice: its first record
    names, records = read_fasta_records(path, ["chr1", "chr2"])
    assert names == ["chr1", "chr2"] and [r.tobytes() for r in records] == [b"GG", b"ACGTAC"]
    assert all(r.dtype == np.uint8 and r.flags["C_CONTIGUOUS"] for r in records)
    assert read_fasta_record(path, "chr2").tobytes() == b"ACGTAC"
    with pytest.raises(KeyError):
        read_fasta_records(path, ["chr1", "chrX"])


def test_error_names_the_line_and_the_rule():
    e = GraphBuildError(7, "unknown", "chrZ")
    assert isinstance(e, ValueError) and (e.line, e.kind) == (7, "unknown")
    assert str(e) == "VCF data line 7: CHROM 'chrZ' is not among the chosen chromosomes"
    assert str(GraphBuildError(0, 3)) == "VCF data line 0: REF differs from the reference"


def test_make_graph_arguments():
    args = build_parser().parse_args(["make_graph", "-r", "ref.fa", "-v", "v.vcf.gz", "-o", "graph", "-n", "chr1,chr2"])
    assert args.func is make_graph and args.chromosomes == "chr1,chr2" and args.variant_to_nodes is None
    assert (args.inflate, args.chunk_bytes) == ("auto", None)
