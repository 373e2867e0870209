"""UniqueVariantKmersFinder on the device against the test-side restatement (tests/spec_unique_variant_kmers.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import spec_unique_variant_kmers as spec
from uvk_cases import bubble_variants

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Pid:
    def __init__(self, base):
        self._base = np.asarray(base, dtype=np.int64)

    def get(self, nodes, offsets):
        return self._base[np.asarray(nodes, dtype=np.int64)] + np.asarray(offsets, dtype=np.int64)


class _V:
    def __init__(self, position, chromosome, line):
        self.position, self.chromosome, self.vcf_line_number = position, chromosome, line


def _index(g, k):
    from graph_kmer_index_amd import DenseKmerFinder, CollisionFreeKmerIndex
    f = DenseKmerFinder(g, k, max_variant_nodes=12)
    f.find()
    return CollisionFreeKmerIndex.from_flat_kmers(f.get_flat_kmers(v="1"), modulo=100003)


def _case(g, k, refs, alts, pos, m=6, lowest=True, chunk_size=None, pid=None, index=None):
    from graph_kmer_index_amd.unique_variant_kmers import UniqueVariantKmersFinder, VariantArrays, VariantToNodesArrays
    index = _index(g, k) if index is None else index
    n = len(pos)
    # line numbers: variant i sits on line 2 i + 1; even lines hold node 0 (skipped)
    ref_nodes = np.zeros(2 * n + 1, np.int64)
    var_nodes = np.zeros(2 * n + 1, np.int64)
    ref_nodes[1::2], var_nodes[1::2] = refs, alts
    lines = np.arange(n) * 2 + 1
    pid = pid or _Pid(g.position_id_base())
    finder = UniqueVariantKmersFinder(g, VariantToNodesArrays(ref_nodes, var_nodes), VariantArrays(pos, 1, lines), k, m,
                                      kmer_index_with_frequencies=index, do_not_choose_lowest_frequency_kmers=not lowest,
                                      use_dense_kmer_finder=True, position_id_index=pid, chunk_size=chunk_size)
    got = finder.find_unique_kmers()
    exp = spec.unique_variant_kmers(g, ref_nodes, var_nodes, pos, lines, k, m, index.get_frequency, lowest, chunk_size,
                                    position_base=pid.get(np.arange(g.n_nodes), np.zeros(g.n_nodes, np.int64)))
    for a, b in zip((got._hashes, got._nodes, got._ref_offsets, got._allele_frequencies), exp):
        assert a.dtype == b.dtype
        assert np.array_equal(a, b)
    return finder, got


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("k,m", [(31, 6), (31, 3), (15, 6)])
def test_snp_graph_matches_spec(seed, k, m):
    from graph_kmer_index_amd.graph import synthetic_snp_graph
    g = synthetic_snp_graph(6000, 120, k=k, seed=seed)
    refs, alts, pos = bubble_variants(g, k)
    assert len(pos) > 50
    _case(g, k, refs, alts, pos, m=m)
    _case(g, k, refs, alts, pos, m=m, lowest=False)


@pytest.mark.parametrize("seed", [3, 4])
def test_indel_graph_matches_spec(seed):
    from graph_kmer_index_amd.graph import synthetic_indel_graph
    g = synthetic_indel_graph(6000, 150, k=31, seed=seed, p_del=0.3, p_ins=0.3)
    refs, alts, pos = bubble_variants(g, 31)
    _case(g, 31, refs, alts, pos)


@pytest.mark.parametrize("seed", [5, 6])
def test_nested_graph_matches_spec(seed):
    from graph_kmer_index_amd.graph import synthetic_nested_graph
    g = synthetic_nested_graph(6000, 150, k=31, seed=seed)
    refs, alts, pos = bubble_variants(g, 31)
    _case(g, 31, refs, alts, pos)


@pytest.mark.parametrize("chunk_size", [None, 1, 3, 7, 40])
def test_shared_nodes_and_chunks(chunk_size):
    """Every variant twice (split multi-allelic lines that share both nodes) and ref nodes shared with a second alt:
    the later ones lose the nodes an earlier variant of the chunk took."""
    from graph_kmer_index_amd.graph import synthetic_snp_graph
    g = synthetic_snp_graph(5000, 100, k=31, seed=9)
    refs, alts, pos = bubble_variants(g, 31)
    o = np.repeat(np.arange(len(pos)), 2)
    refs, alts, pos = refs[o], alts[o], pos[o]
    finder, got = _case(g, 31, refs, alts, pos, chunk_size=chunk_size)
    assert (finder.last_serial_variants > 0) == (chunk_size != 1)      # one variant per chunk shares nothing


def test_empty_and_skipped():
    from graph_kmer_index_amd.graph import synthetic_snp_graph
    from graph_kmer_index_amd.unique_variant_kmers import UniqueVariantKmersFinder, VariantToNodesArrays
    g = synthetic_snp_graph(3000, 40, k=31, seed=2)
    index = _index(g, 31)
    pid = _Pid(g.position_id_base())
    for variants in ([], [_V(500, 1, 0), _V(900, 1, 1)]):
        f = UniqueVariantKmersFinder(g, VariantToNodesArrays(np.zeros(2, np.int64), np.array([5, 0])), variants, 31,
                                     kmer_index_with_frequencies=index, use_dense_kmer_finder=True, position_id_index=pid)
        flat = f.find_unique_kmers()
        assert len(flat._hashes) == 0 and flat._hashes.dtype == np.uint64


def test_object_variants_and_device_output_agree():
    from graph_kmer_index_amd.graph import synthetic_snp_graph
    from graph_kmer_index_amd.unique_variant_kmers import UniqueVariantKmersFinder, VariantToNodesArrays
    g = synthetic_snp_graph(5000, 80, k=31, seed=4)
    refs, alts, pos = bubble_variants(g, 31)
    index = _index(g, 31)
    pid = _Pid(g.position_id_base())
    v2n = VariantToNodesArrays(refs, alts)
    variants = [_V(int(p), "1", i) for i, p in enumerate(pos)]
    f = UniqueVariantKmersFinder(g, v2n, variants, 31, kmer_index_with_frequencies=index, use_dense_kmer_finder=True,
                                 position_id_index=pid)
    flat = f.find_unique_kmers()
    d = f.find_unique_kmers_on_device()
    back = d.to_flat_kmers()
    for a, b in zip((flat._hashes, flat._nodes, flat._ref_offsets, flat._allele_frequencies),
                    (back._hashes, back._nodes, back._ref_offsets, back._allele_frequencies)):
        assert np.array_equal(a, b)
    assert len(flat._hashes) > 0


def test_start_outside_linear_reference_raises():
    from graph_kmer_index_amd.graph import synthetic_snp_graph
    from graph_kmer_index_amd.unique_variant_kmers import UniqueVariantKmersFinder, VariantToNodesArrays
    g = synthetic_snp_graph(3000, 40, k=31, seed=2)
    f = UniqueVariantKmersFinder(g, VariantToNodesArrays(np.array([3]), np.array([4])), [_V(10, 1, 0)], 31,
                                 kmer_index_with_frequencies=_index(g, 31), use_dense_kmer_finder=True,
                                 position_id_index=_Pid(g.position_id_base()))
    with pytest.raises(ValueError, match="variant 0"):
        f.find_unique_kmers()


def _run_cli(args, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    subprocess.run([sys.executable, "-m", "graph_kmer_index_amd.command_line_interface"] + args, check=True, env=env,
                   cwd=str(tmp_path))


def test_cli_equals_api_and_make_reverse(tmp_path):
    from graph_kmer_index_amd import ReverseKmerIndex, FlatKmers
    from graph_kmer_index_amd.graph import synthetic_snp_graph
    from graph_kmer_index_amd.unique_variant_kmers import UniqueVariantKmersFinder, VariantArrays, VariantToNodesArrays
    g = synthetic_snp_graph(5000, 80, k=31, seed=7)
    refs, alts, pos = bubble_variants(g, 31)
    o = np.repeat(np.arange(len(pos)), 2)               # shared nodes, so that -c matters
    refs, alts, pos = refs[o], alts[o], pos[o]
    index = _index(g, 31)
    g.to_file(str(tmp_path / "graph.npz"))
    index.to_file(str(tmp_path / "index"))
    VariantToNodesArrays(refs, alts).to_file(str(tmp_path / "v2n.npz"))
    with open(tmp_path / "v.vcf", "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n")
        for p in pos:
            f.write("1\t%d\t.\tA\tC\n" % p)
    _run_cli(["make_unique_variant_kmers", "-g", "graph.npz", "-V", "v2n.npz", "-k", "31", "-i", "index.npz", "-D",
              "True", "-v", "v.vcf", "-c", "5", "-t", "4", "-o", "uvk"], tmp_path)
    cli = np.load(tmp_path / "uvk.npz")
    f = UniqueVariantKmersFinder(g, VariantToNodesArrays(refs, alts), VariantArrays(pos, "1", np.arange(len(pos))), 31,
                                 kmer_index_with_frequencies=index, use_dense_kmer_finder=True,
                                 position_id_index=_Pid(g.position_id_base()), chunk_size=5)
    api = f.find_unique_kmers()
    for key, a in (("hashes", api._hashes), ("nodes", api._nodes), ("ref_offsets", api._ref_offsets),
                   ("allele_frequencies", api._allele_frequencies)):
        assert cli[key].dtype == a.dtype and np.array_equal(cli[key], a)
    _run_cli(["make_reverse", "-f", "uvk.npz", "-o", "rev"], tmp_path)
    ReverseKmerIndex.from_flat_kmers(FlatKmers.from_file(str(tmp_path / "uvk.npz"))).to_file(str(tmp_path / "rev_api"))
    a, b = np.load(tmp_path / "rev.npz"), np.load(tmp_path / "rev_api.npz")
    assert sorted(a.files) == sorted(b.files)
    for key in a.files:
        assert np.array_equal(a[key], b[key])


def test_mid_size_graph_matches_spec():
    from graph_kmer_index_amd.graph import synthetic_snp_graph
    g = synthetic_snp_graph(20_000_000, 30_000, k=31, seed=11)
    refs, alts, pos = bubble_variants(g, 31)
    assert len(pos) > 29_000
    from graph_kmer_index_amd import DenseKmerFinder, CollisionFreeKmerIndex
    f = DenseKmerFinder(g, 31, max_variant_nodes=4)
    f.find()
    index = CollisionFreeKmerIndex.from_flat_kmers(f.get_flat_kmers(v="1"), modulo=20_000_003)
    _case(g, 31, refs, alts, pos, index=index)
