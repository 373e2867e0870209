"""Host side of UniqueVariantKmersFinder (no GPU): VCF reader, positional mapping, selection rules, CLI options and the
modes that are refused."""
import os

import numpy as np
import pytest

from graph_kmer_index_amd.graph import GraphArrays
from graph_kmer_index_amd.unique_variant_kmers import (LinearReference, UniqueVariantKmersFinder, VariantArrays,
                                                       SUMMARY_DTYPE, choose_position, start_distances)
from graph_kmer_index_amd.collision_free_kmer_index import CollisionFreeKmerIndex
import spec_unique_variant_kmers as spec


def _graph():
    # 0:ACGTACGTAC (10) -> 1:G | 2:T -> 3:'' (dummy, linear) -> 4:TTTTTTTTTTTT (12); second chromosome 5:CCCCC
    return GraphArrays.from_dicts({0: "ACGTACGTAC", 1: "G", 2: "T", 3: "", 4: "TTTTTTTTTTTT", 5: "CCCCC"},
                                  {0: [1, 2], 1: [3], 2: [3], 3: [4]}, [0, 1, 3, 4, 5],
                                  chromosome_start_nodes=[0, 5])


def test_start_distances():
    assert start_distances(31) == [26, 22, 18, 14, 10, 6, 2]
    assert start_distances(7) == [2]
    assert start_distances(4) == []


def test_vcf_reader_numbers_data_lines(tmp_path):
    p = tmp_path / "v.vcf"
    p.write_text("##x\n#CHROM\tPOS\tID\n1\t100\t.\tA\tC\nchr2\t7\t.\tG\tT\n\n2\t9\n")
    v = VariantArrays.from_vcf(str(p))
    assert v.positions.tolist() == [100, 7, 9]
    assert v.chromosomes.tolist() == ["1", "chr2", "2"]
    assert v.line_numbers.tolist() == [0, 1, 2]


def test_linear_reference_mapping_and_errors():
    g = _graph()
    lin = LinearReference(g, g)
    nodes, offs = lin.node_and_offset([0, 9, 10, 11, 22, 23, 27])
    assert nodes.tolist() == [0, 0, 1, 4, 4, 5, 5] and offs.tolist() == [0, 9, 0, 0, 11, 0, 4]
    assert lin.chromosome_offset(1) == 0 and lin.chromosome_offset("2") == 23
    for bad in ([-1], [28]):
        with pytest.raises(ValueError):
            lin.node_and_offset(bad)
    with pytest.raises(ValueError):
        lin.chromosome_offset("chrX")
    for x in (0, 5, 10, 11, 27):
        assert spec.node_at_ref_offset(g, x) == tuple(int(a[0]) for a in lin.node_and_offset([x]))


def _summaries(rows):
    s = np.zeros(len(rows), SUMMARY_DTYPE)
    for i, r in enumerate(rows):
        s[i] = r
    return s


def test_choose_position_rules():
    # (n_ref, n_alt, f_ref, f_alt, flags)
    s = _summaries([(1, 1, 5, 5, 0), (1, 1, 3, 1, 1), (1, 1, 2, 2, 0), (1, 1, 1, 0, 0), (1, 1, 0, 0, 0)])
    assert choose_position(s, 3, True) == 3          # shared at 1 skipped, break after the score-1 position
    assert choose_position(s, 3, False) == 0
    assert choose_position(s, 2, True) == 1          # without the ref node nothing is shared: alt score 1 at j=1
    s = _summaries([(1, 1, 4, 4, 1), (1, 1, 4, 4, 1)])
    assert choose_position(s, 3, True) == 1          # the last position is always valid


def test_refused_modes():
    g = _graph()
    idx = CollisionFreeKmerIndex()
    with pytest.raises(NotImplementedError, match="use_dense_kmer_finder=True"):
        UniqueVariantKmersFinder(g, None, [], kmer_index_with_frequencies=idx, position_id_index=object())
    with pytest.raises(NotImplementedError, match="use_simple"):
        UniqueVariantKmersFinder(g, None, [], kmer_index_with_frequencies=idx, use_dense_kmer_finder=True,
                                 position_id_index=object(), use_simple=True)
    with pytest.raises(NotImplementedError, match="CollisionFreeKmerIndex"):
        UniqueVariantKmersFinder(g, None, [], kmer_index_with_frequencies=object(), use_dense_kmer_finder=True,
                                 position_id_index=object())


def test_cli_options_and_refusals(tmp_path):
    from graph_kmer_index_amd.command_line_interface import build_parser
    p = build_parser()
    a = p.parse_args(["make_unique_variant_kmers", "-g", "g", "-V", "v", "-k", "31", "-i", "i", "-p", "p", "-D", "True",
                      "-o", "o", "-v", "x.vcf", "-t", "3", "-c", "17", "-m", "4", "-d", "True", "-S", "False",
                      "-N", "n", "-H", "h", "-I", "c"])
    assert (a.kmer_size, a.n_threads, a.chunk_size, a.max_variant_nodes) == (31, 3, 17, 4)
    assert a.use_dense_kmer_finder and a.do_not_choose_lowest_frequency_kmers and not a.simple
    d = p.parse_args(["make_unique_variant_kmers", "-g", "g", "-V", "v", "-k", "31", "-o", "o"])
    assert (d.chunk_size, d.max_variant_nodes, d.n_threads, d.use_dense_kmer_finder) == (10000, 6, 1, False)
    with pytest.raises(NotImplementedError, match="-D True"):
        d.func(d)
    a.use_dense_kmer_finder = True
    with pytest.raises(NotImplementedError, match="-N"):
        a.func(a)
    r = p.parse_args(["make_reverse", "-f", "flat.npz", "-o", "rev"])
    assert r.flat_index == "flat.npz" and r.out_file_name == "rev"


def test_variant_to_nodes_loader(tmp_path):
    from graph_kmer_index_amd.unique_variant_kmers import load_variant_to_nodes, VariantToNodesArrays
    VariantToNodesArrays(np.array([0, 3]), np.array([0, 4])).to_file(str(tmp_path / "v2n.npz"))
    for name in ("v2n.npz", "v2n"):
        v = load_variant_to_nodes(str(tmp_path / name))
        assert v.ref_nodes.tolist() == [0, 3] and v.var_nodes.tolist() == [0, 4]
    with pytest.raises(FileNotFoundError):
        load_variant_to_nodes(str(tmp_path / "missing.npz"))
