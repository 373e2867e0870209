"""UniqueVariantKmersFinder on the device against the reference's own output (tests/golden/uvk_reference.json.gz), and
against the CPU restatement on seeded graphs with planted repeats, shared-hash deletions and dense SNP clusters."""
import numpy as np
import pytest

import spec_unique_variant_kmers as spec
from uvk_cases import planted_chromosome, planted_graph
from uvk_golden import load_cases, case_graph, case_index_flat, expected

pytestmark = pytest.mark.gpu
CASES = load_cases()


class _Pid:
    def __init__(self, base):
        self._base = np.asarray(base, dtype=np.int64)

    def get(self, nodes, offsets):
        return self._base[np.asarray(nodes, dtype=np.int64)] + np.asarray(offsets, dtype=np.int64)


def _finder(g, ref, var, variants, k, m, index, lowest, chunk_size, graph=None):
    from graph_kmer_index_amd.unique_variant_kmers import UniqueVariantKmersFinder, VariantToNodesArrays
    return UniqueVariantKmersFinder(g if graph is None else graph, VariantToNodesArrays(ref, var), variants, k, m,
                                    kmer_index_with_frequencies=index, do_not_choose_lowest_frequency_kmers=not lowest,
                                    use_dense_kmer_finder=True, position_id_index=_Pid(g.position_id_base()),
                                    chunk_size=chunk_size)


def _cols(flat):
    return flat._hashes, flat._nodes, flat._ref_offsets, flat._allele_frequencies


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_equals_reference(case):
    from graph_kmer_index_amd import CollisionFreeKmerIndex
    from graph_kmer_index_amd.unique_variant_kmers import VariantArrays
    g = case_graph(case)
    index = CollisionFreeKmerIndex.from_flat_kmers(case_index_flat(case), modulo=case["index"]["modulo"])
    v = case["variants"]
    f = _finder(g, case["ref_nodes"], case["var_nodes"], VariantArrays(v["positions"], v["chromosomes"], v["lines"]),
                case["k"], case["max_variant_nodes"], index, case["lowest"], case["chunk_size"])
    got = f.find_unique_kmers()
    for a, b in zip(_cols(got), expected(case)):
        assert a.dtype == b.dtype and np.array_equal(a, b)


def _planted(seed, k, **kw):
    from graph_kmer_index_amd import DenseKmerFinder, CollisionFreeKmerIndex
    from graph_kmer_index_amd.graph import GraphArrays
    from graph_kmer_index_amd.flat_kmers import FlatKmers
    rng = np.random.default_rng(seed)
    ns, ed, lin, starts, variants = planted_graph([planted_chromosome(rng, **kw)])
    g = GraphArrays.from_dicts(ns, ed, lin, chromosome_start_nodes=starts)
    f = DenseKmerFinder(g, k, max_variant_nodes=4, only_save_one_node_per_kmer=True)
    f.find()
    fl = f.get_flat_kmers(v="1")
    keep = np.asarray(fl._hashes) % 3 != 0
    index = CollisionFreeKmerIndex.from_flat_kmers(
        FlatKmers(fl._hashes[keep], fl._nodes[keep], fl._ref_offsets[keep], fl._allele_frequencies[keep]), modulo=20011)
    return g, index, variants


@pytest.mark.parametrize("seed", [21, 22, 23])
@pytest.mark.parametrize("k", [31, 19])
def test_planted_graphs_match_spec_and_modes_differ(seed, k):
    from graph_kmer_index_amd.unique_variant_kmers import VariantArrays
    g, index, variants = _planted(seed, k, length=8000, n_snps=60, n_dels=6, n_repeats=25)
    pos = np.array([p for p, _, _, _ in variants])
    ref = np.array([r for _, _, r, _ in variants])
    alt = np.array([a for _, _, _, a in variants])
    lines = np.arange(len(pos))
    outs = []
    for lowest in (True, False):
        got = _finder(g, ref, alt, VariantArrays(pos, 1, lines), k, 6, index, lowest, None).find_unique_kmers()
        exp = spec.unique_variant_kmers(g, ref, alt, pos, lines, k, 6, index.get_frequency, lowest)
        for a, b in zip(_cols(got), exp):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        outs.append(got)
    assert not (len(outs[0]._hashes) == len(outs[1]._hashes) and np.array_equal(outs[0]._hashes, outs[1]._hashes))


def test_accessor_check_agrees_and_disagrees():
    from graph_kmer_index_amd.unique_variant_kmers import VariantArrays, LinearReference
    g, index, variants = _planted(31, 31, length=3000, n_snps=20)
    lin = LinearReference(g, g)

    class WithAccessors:
        """An obgraph-like graph object with the three positional accessors (shift: a deliberate disagreement)."""
        def __init__(self, shift):
            self.shift = shift
            self.chromosome_start_nodes = g.chromosome_start_nodes
            self.node_to_ref_offset = g.node_to_ref_offset

        def __getattr__(self, name):
            return getattr(g, name)

        def convert_chromosome_ref_offset_to_graph_ref_offset(self, offset, chromosome):
            return lin.chromosome_offset(chromosome) + offset

        def get_node_at_ref_offset(self, x):
            return int(lin.node_and_offset([x])[0][0])

        def get_node_offset_at_ref_offset(self, x):
            return int(lin.node_and_offset([x])[1][0]) + self.shift

    pos = np.array([p for p, _, _, _ in variants])
    ref = np.array([r for _, _, r, _ in variants])
    alt = np.array([a for _, _, _, a in variants])
    va = VariantArrays(pos, 1, np.arange(len(pos)))
    plain = _finder(g, ref, alt, va, 31, 6, index, True, None).find_unique_kmers()
    ok = _finder(g, ref, alt, va, 31, 6, index, True, None, graph=WithAccessors(0)).find_unique_kmers()
    assert np.array_equal(plain._hashes, ok._hashes)
    with pytest.raises(ValueError, match="disagree"):
        _finder(g, ref, alt, va, 31, 6, index, True, None, graph=WithAccessors(1)).find_unique_kmers()


def test_k_below_5_raises():
    from graph_kmer_index_amd.unique_variant_kmers import VariantArrays
    g, index, variants = _planted(32, 31, length=2000, n_snps=5)
    p, _, r, a = variants[0]
    with pytest.raises(ValueError, match="no start position"):
        _finder(g, [r], [a], VariantArrays([p], 1, [0]), 4, 6, index, True, None).find_unique_kmers()
