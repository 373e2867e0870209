"""The graph build on the device (graph_files.py, csrc/gki_graph_build.hip) against the plain-Python rules of
tests/spec_graph_build.py: every array, on every named case; the refused inputs; pieces cut anywhere, from plain, BGZF
and gzip files; and the command line followed by the finder and the variant k-mers on what it wrote."""
import gzip

import numpy as np
import pytest

import spec_graph_build as spec
from graph_build_cases import ERROR_CASES, GOOD_CASES, deletion, insertion, line, other_base, random_reference, snp, vcf

pytestmark = pytest.mark.gpu

GRAPH_ARRAYS = ("node_size", "seq", "edge_start", "edges", "rev_start", "rev_edges", "is_ref", "allele_freq", "exists",
                "node_to_ref_offset")
_SPEC = {}


def spec_of(name):
    if name not in _SPEC:
        _SPEC[name] = spec.build(*GOOD_CASES[name])
    return _SPEC[name]


def assert_equals_spec(built, want):
    g = built.graph
    for key in GRAPH_ARRAYS:
        got, exp = np.asarray(getattr(g, key)), getattr(want, key)
        assert got.dtype == exp.dtype and np.array_equal(got, exp), key
    assert np.array_equal(g.seq_start, np.concatenate([[0], np.cumsum(want.node_size, dtype=np.int64)]))
    assert g._chromosome_start_nodes == want.chromosome_start_nodes and g.first_node == 1
    for key in ("ref_nodes", "var_nodes"):
        got = getattr(built.variant_to_nodes, key)
        assert got.dtype == np.uint32 and np.array_equal(got, getattr(want, key)), key
    assert built.line_status.dtype == np.uint8 and np.array_equal(built.line_status, want.line_status)


@pytest.mark.parametrize("name", sorted(GOOD_CASES))
def test_case_equals_spec(name):
    from graph_kmer_index_amd.graph_files import build_graph
    reference, text = GOOD_CASES[name]
    assert_equals_spec(build_graph(reference, text), spec_of(name))


def test_allele_frequencies_and_chosen_chromosomes():
    from graph_kmer_index_amd.graph_files import build_graph
    reference, text = GOOD_CASES["mixed_random_two_chromosomes"]
    n = len(spec_of("mixed_random_two_chromosomes").line_status)
    rng = np.random.default_rng(3)
    af = (rng.uniform(0.01, 0.99, n), rng.uniform(0.01, 0.99, n))
    assert_equals_spec(build_graph(reference, text, allele_frequencies=af), spec.build(reference, text, allele_frequencies=af))
    more = dict(reference, unused=b"ACGTACGT")
    assert_equals_spec(build_graph(more, text, chromosomes=["a", "b"]), spec_of("mixed_random_two_chromosomes"))
    assert_equals_spec(build_graph(more, text, chromosomes=["a", "b", "unused"]),
                       spec.build(more, text, chromosomes=["a", "b", "unused"]))


@pytest.mark.parametrize("name", sorted(ERROR_CASES))
def test_error_case_names_the_line(name):
    from graph_kmer_index_amd.graph_files import GraphBuildError, build_graph
    reference, text, line, _ = ERROR_CASES[name]
    with pytest.raises(spec.BuildError) as want:
        spec.build(reference, text)
    with pytest.raises(ValueError) as e:
        build_graph(reference, text)
    assert isinstance(e.value, GraphBuildError) and e.value.line == want.value.line == line
    assert "data line %d:" % line in str(e.value)


def write_fasta(path, reference, width=61):
    with open(path, "wb") as f:
        for name, letters in reference.items():
            f.write(b">%s some description\n" % name.encode())
            for a in range(0, len(letters), width):
                f.write(letters[a:a + width] + b"\n")


@pytest.fixture(scope="module", params=["lines_2049", "mixed_random", "mixed_random_two_chromosomes"])
def case_files(request, tmp_path_factory):
    from graph_kmer_index_amd import bgzf
    d = tmp_path_factory.mktemp("graph_build_" + request.param)
    reference, text = GOOD_CASES[request.param]
    paths = {"fasta": str(d / "ref.fa"), "plain": str(d / "v.vcf"), "bgzf": str(d / "v_bgzf.vcf.gz"),
             "gzip": str(d / "v_gzip.vcf.gz")}
    write_fasta(paths["fasta"], reference)
    with open(paths["plain"], "wb") as f:
        f.write(text)
    bgzf.write_bgzf(paths["bgzf"], text, block_size=777)                # lines span members
    with open(paths["gzip"], "wb") as f:
        f.write(gzip.compress(text))
    return request.param, paths


@pytest.mark.parametrize("encoding", ["plain", "bgzf", "gzip"])
@pytest.mark.parametrize("chunk_bytes", [64, 1, None])                  # 1: a cut after every line of the host routes
def test_pieces_cut_anywhere(case_files, encoding, chunk_bytes):
    from graph_kmer_index_amd.graph_files import build_graph_from_files
    name, paths = case_files
    built = build_graph_from_files(paths["fasta"], paths[encoding], chunk_bytes=chunk_bytes)
    assert_equals_spec(built, spec_of(name))


def test_error_line_numbers_carry_across_pieces(tmp_path):
    from graph_kmer_index_amd.graph_files import GraphBuildError, build_graph_from_files
    r = random_reference(400, 21)
    lines = [snp("1", r, 5 + 3 * i) for i in range(100)]
    write_fasta(str(tmp_path / "ref.fa"), {"1": r})
    for bad, kind in ((snp("1", r, 20), "decreasing"), (line("1", 350, other_base(r[349]), r[349:350]), 3)):
        with open(str(tmp_path / "v.vcf"), "wb") as f:
            f.write(vcf(lines + [bad]))
        with pytest.raises(GraphBuildError) as e:
            build_graph_from_files(str(tmp_path / "ref.fa"), str(tmp_path / "v.vcf"), chunk_bytes=64)
        assert (e.value.line, e.value.kind) == (100, kind)


def test_command_line_then_finder_and_variant_kmers(tmp_path):
    from graph_kmer_index_amd import DenseKmerFinder
    from graph_kmer_index_amd.command_line_interface import build_parser, load_graph
    from graph_kmer_index_amd.graph import GraphArrays
    from graph_kmer_index_amd.unique_variant_kmers import (VariantArrays, VariantToNodesArrays, find_kmers_over_variants,
                                                           load_variant_to_nodes)
    from gpu_util import assert_same_records, finder_cols
    r = random_reference(4000, 31)
    makers = (snp, lambda c, ref, p: deletion(c, ref, p, 3), lambda c, ref, p: insertion(c, ref, p, b"GAT"))
    lines = [makers[i % 3]("1", r, pos) for i, pos in enumerate(range(100, 3900, 95))]
    text = vcf(lines)
    fasta, vcf_path, out = str(tmp_path / "ref.fa"), str(tmp_path / "v.vcf.gz"), str(tmp_path / "graph")
    write_fasta(fasta, {"other": b"ACGT" * 10, "1": r})        # the other commands know chromosomes by number
    with open(vcf_path, "wb") as f:
        f.write(gzip.compress(text))
    args = build_parser().parse_args(["make_graph", "-r", fasta, "-v", vcf_path, "-o", out, "-n", "1"])
    args.func(args)
    graph, v2n = load_graph(out), load_variant_to_nodes(out + ".variant_to_nodes")
    want = spec.build({"1": r}, text)
    want_graph = GraphArrays(want.node_size, want.seq, want.edge_start, want.edges, want.is_ref, want.allele_freq, want.exists,
                             1, want.chromosome_start_nodes, want.node_to_ref_offset)
    assert np.array_equal(v2n.ref_nodes, want.ref_nodes) and np.array_equal(v2n.var_nodes, want.var_nodes)
    assert np.all(want.line_status == 0)

    def records(g):
        f = DenseKmerFinder(g, 31, max_variant_nodes=5, only_save_one_node_per_kmer=True)
        f.find()
        return finder_cols(f)
    assert_same_records(records(graph), records(want_graph))
    variants = VariantArrays.from_vcf(vcf_path)
    got = find_kmers_over_variants(graph, v2n, variants, 31)
    exp = find_kmers_over_variants(want_graph, VariantToNodesArrays(want.ref_nodes, want.var_nodes), variants, 31)
    assert len(got._hashes) > 0
    for key in ("_hashes", "_nodes", "_ref_offsets", "_allele_frequencies"):
        assert np.array_equal(getattr(got, key), getattr(exp, key)), key
