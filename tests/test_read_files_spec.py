"""The reads-file semantics (tests/spec_read_files.py) pinned without a GPU: against the hashes the reference's
ReadKmers.from_fasta_file yields (recorded in tests/golden/read_files_reference.json.gz, and run live where the reference
tree is present), FASTQ against its FASTA rewriting, and the chunk-cutting rule at every chunk size."""
import gzip
import io
import json
import logging
import os
import sys

import numpy as np
import pytest

import read_file_cases as cases
import spec_read_files as spec
from read_side_ref import hash_reads_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "read_files_reference.json.gz")
T, S = 4096, 2048          # the sizes tests/test_gpu_read_files.py takes from the kernels


@pytest.fixture(scope="module")
def golden():
    with gzip.open(GOLDEN, "rt") as fh:
        return json.load(fh)


def per_read(hashes, out_start):
    return [hashes[a:b].tolist() for a, b in zip(out_start[:-1], out_start[1:])]


def test_golden_holds_every_case_and_few_undefined_reads(golden):
    assert set(golden) == set(cases.GOLDEN_CASES)
    n = undefined = 0
    for name, by_k in golden.items():
        assert set(by_k) == {str(k) for k in cases.GOLDEN_KS}
        for k, e in by_k.items():
            assert len(e["forward"]) == len(e["reverse"])
            assert [x is None for x in e["forward"]] == [x is None for x in e["reverse"]]
            assert any(x is not None for x in e["forward"]), (name, k)        # every case holds a defined read
            n += len(e["forward"])
            undefined += sum(x is None for x in e["forward"])
    assert 0 < undefined <= n // 5, (undefined, n)


@pytest.mark.parametrize("name", sorted(cases.GOLDEN_CASES))
@pytest.mark.parametrize("k", cases.GOLDEN_KS)
def test_spec_reads_hash_to_the_reference(golden, name, k):
    data = cases.GOLDEN_CASES[name]
    assert set(data) <= set(b"ACGTacgt>\r\n") | set(spec.STRIP) | set(b"abcdefghijklmnopqrstuvwxyz0123456789 ")
    reads, n_lines, n_bad = spec.parse(data, "fasta")
    assert all(set(r) <= set(b"ACGTacgt") and len(r) > 0 for r in reads)
    e = golden[name][str(k)]
    assert len(reads) == len(e["forward"])
    letters, read_start = spec.layout(reads)
    for strand, key in ((0, "forward"), (1, "reverse")):
        got = per_read(*hash_reads_ref(letters, read_start, k, strand))
        for r, (g, want) in enumerate(zip(got, e[key])):
            if want is None:                         # shorter than k: no k-mers here, undefined in the reference
                assert len(reads[r]) < k and g == []
            else:
                assert g == want, (name, k, key, r)


@pytest.mark.reference
def test_golden_equals_a_fresh_reference_run(golden):
    saved = list(sys.path)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    logging.disable(logging.CRITICAL)
    try:
        import make_golden_read_files
        assert make_golden_read_files.run_all() == golden
    finally:
        logging.disable(logging.NOTSET)
        sys.path[:] = saved


@pytest.mark.parametrize("name", sorted(cases.FASTQ_CASES))
def test_fastq_equals_its_fasta_rewriting(name):
    data, records = cases.FASTQ_CASES[name]
    reads, n_lines, n_bad = spec.parse(data, "fastq")
    assert n_bad == 0
    assert n_lines == spec.n_lines_of(data)
    want, _, _ = spec.parse(cases.fasta_rewriting(records), "fasta")
    assert reads == want and len(reads) == len(records)
    assert spec.detect_format(data) == "fastq"


def test_fastq_record_shape():
    assert spec.parse(cases.BAD_THIRD_LINE, "fastq")[2] == 1
    assert spec.parse(b"@a\nAC\n+\n>>\nAC\n", "fastq")[2] == 1          # a fifth line that is no name line
    assert spec.parse(b"\n", "fastq") == ([], 1, 1)
    # the same lines are in place when the phase says where the buffer begins
    assert spec.parse(b"+\n@@\n@b\nGT\n", "fastq", 2) == ([b"GT"], 4, 0)


def test_line_counts_and_small_files():
    assert spec.parse(b"", "fasta") == ([], 0, 0)
    assert spec.parse(b"A", "fasta") == ([b"A"], 1, 0)
    assert spec.parse(b"\n", "fasta") == ([b""], 1, 0)
    assert spec.parse(b" >x\n>y\n", "fasta") == ([b">x"], 2, 0)
    assert spec.parse(b">a\r\nAC\r\n\r\n", "fasta") == ([b"AC", b""], 3, 0)
    assert spec.parse(b"\x1cAC\x1f\n\x00A\x08\n", "fasta") == ([b"AC", b"\x00A\x08"], 2, 0)
    assert spec.detect_format(b"") == "fasta" and spec.detect_format(b">") == "fasta"
    with pytest.raises(ValueError):
        spec.detect_format(b"ACGT\n")


def _small_files():
    out = {("fasta", name): data for name, data in cases.GOLDEN_CASES.items() if name != "stream"}
    out.update({("fasta", name): data for name, data in cases.PARSE_CASES.items()})
    out.update({("fastq", name): data for name, (data, _) in cases.FASTQ_CASES.items()})
    out[("fastq", "bad_third_line")] = cases.BAD_THIRD_LINE
    return out


@pytest.mark.parametrize("fmt,name", sorted(_small_files()))
def test_every_chunk_size_reproduces_the_whole_file(fmt, name):
    data = _small_files()[(fmt, name)]
    whole = spec.parse(data, fmt)
    for chunk_bytes in range(1, len(data) + 2):
        pieces = spec.cut_chunks(data, chunk_bytes)
        assert b"".join(pieces) == data
        assert all(p.endswith(b"\n") for p in pieces[:-1]) and all(pieces)
        reads, n_lines, n_bad, phases = spec.parse_chunked(data, fmt, chunk_bytes)
        assert (reads, n_lines, n_bad) == whole, chunk_bytes
        lines_before = np.cumsum([0] + [spec.n_lines_of(p) for p in pieces[:-1]])
        assert phases == [int(x) % 4 for x in lines_before[:len(pieces)]]
        if chunk_bytes > len(data):
            assert pieces == ([data] if data else [])


def test_chunks_grow_past_a_long_line():
    data = cases.boundary_cases(T, S)["tile_without_newline"]
    for chunk_bytes in (1, 7, 64, T, T + 1):
        pieces = spec.cut_chunks(data, chunk_bytes)
        assert b"".join(pieces) == data and max(len(p) for p in pieces) > 2 * T
        assert spec.parse_chunked(data, "fasta", chunk_bytes)[:3] == spec.parse(data, "fasta")


@pytest.mark.parametrize("chunk_bytes", [1, 2, 7, 64, 1000, 10 ** 6])
def test_the_package_cuts_a_stream_as_the_spec_does(chunk_bytes):
    """graph_kmer_index_amd.read_files.iter_line_chunks over a file object (host code, no device) against cut_chunks."""
    from graph_kmer_index_amd.read_files import detect_format, iter_line_chunks
    files = list(_small_files().values()) + [cases.GOLDEN_CASES["stream"]]
    for data in files:
        assert list(iter_line_chunks(io.BytesIO(data), chunk_bytes)) == spec.cut_chunks(data, chunk_bytes)

    class Dribble(io.BytesIO):                       # a stream that answers a read with fewer bytes than asked for
        def read(self, n=-1):
            return super().read(min(n, 3) if n and n > 0 else n)
    data = cases.GOLDEN_CASES["crlf"]
    assert list(iter_line_chunks(Dribble(data), chunk_bytes)) == spec.cut_chunks(data, chunk_bytes)
    assert detect_format(b"") == "fasta" and detect_format(b">x") == "fasta" and detect_format(b"@x") == "fastq"
    with pytest.raises(ValueError):
        detect_format(b"ACGT")


def test_boundary_files_have_the_lines_they_are_named_for():
    b = cases.boundary_cases(T, S)
    assert spec.parse(b["T_plus_3_newlines"], "fasta") == ([b""] * (T + 3), T + 3, 0)
    assert spec.parse(b["%d_lines_of_A" % (2 * S + 1)], "fasta") == ([b"A"] * (2 * S + 1), 2 * S + 1, 0)
    reads, n_lines, _ = spec.parse(b["line_of_2T_plus_3"], "fasta")
    assert [len(r) for r in reads] == [2 * T + 3, 8]
    reads, _, _ = spec.parse(b["whitespace_line_over_a_tile"], "fasta")
    assert reads == [b"", b"ACGT", b"AC"]


def test_cli_parser_accepts_map():
    from graph_kmer_index_amd.command_line_interface import build_parser, map_reads_file
    args = build_parser().parse_args(["map", "-i", "index", "-f", "reads.fq.gz", "-o", "counts"])
    assert args.func is map_reads_file
    assert (args.kmer_size, args.n_nodes, args.include_reverse_complement, args.format, args.chunk_bytes) == \
        (31, None, True, None, None)
    assert args.max_hits == 2 ** 62
    args = build_parser().parse_args(["map", "-i", "index", "-f", "r.fa", "-o", "c", "-k", "5", "-n", "40", "-r", "False",
                                      "-m", "10", "-c", "4096", "-F", "fastq", "-t", "8"])
    assert (args.kmer_size, args.n_nodes, args.include_reverse_complement, args.max_hits, args.chunk_bytes, args.format) == \
        (5, 40, False, 10, 4096, "fastq")
