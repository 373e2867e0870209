"""-m gpu: the split-layout interior stream (k_emit_interior_dense and what it leaves to k_emit_interior_dense_rest)
against the by-node layout of the same run, record by record: the split output holds the same multiset of records,
its interior section ordered by position, on graphs chosen for the block mapping's corner cases."""
import numpy as np
import pytest

from graph_kmer_index_amd import DenseKmerFinder, CriticalGraphPaths
from graph_kmer_index_amd.graph import (synthetic_indel_graph, synthetic_linear_graph, synthetic_nested_graph,
                                        synthetic_snp_graph)
from oracle import oracle

pytestmark = pytest.mark.gpu
IB = 4096          # records per output block of the dense interior kernel


def _columns(d, f):
    f.synchronize()
    fl = d.to_flat_kmers()
    return fl._hashes, fl._nodes, fl._ref_offsets, fl._allele_frequencies


def _check_split(f):
    """Split layout against the by-node layout of the same finder and run; returns the interior record count."""
    want = _columns(f.find_flat_on_device(split_layout=False), f)
    got = _columns(f.find_flat_on_device(split_layout=True), f)
    n_int = f.interior_records()
    assert len(got[0]) == len(want[0])
    og = np.lexsort((got[3], got[1], got[0], got[2]))
    ow = np.lexsort((want[3], want[1], want[0], want[2]))
    for a, b in zip(got, want):
        assert np.array_equal(a[og], b[ow])
    # interior records: one window per position, written by position
    assert np.all(np.diff(got[2][:n_int].astype(np.int64)) > 0)
    return n_int


def _check_against_oracle(g, k, f, crit=None, **kw):
    exp = oracle.find(g, k, crit, True, 5, **kw)
    got = _columns(f.find_flat_on_device(split_layout=True), f)
    pos = g.position_id_base()[exp["start_nodes"]] + exp["start_offsets"]
    o1 = np.lexsort((got[0], got[2], got[1]))
    o2 = np.lexsort((exp["kmers"].astype(np.uint64), pos.astype(np.uint64), exp["nodes"].astype(np.uint32)))
    assert np.array_equal(got[0][o1], exp["kmers"].astype(np.uint64)[o2])
    assert np.array_equal(got[1][o1], exp["nodes"].astype(np.uint32)[o2])
    assert np.array_equal(got[2][o1], pos.astype(np.uint64)[o2])


@pytest.mark.parametrize("n_bases", [31 + 40, 30 + IB, 30 + 3 * IB, 30 + 3 * IB + 1, 30 + 3 * IB - 1, 200000])
def test_linear_runs_longer_than_a_block_and_block_aligned_ends(n_bases):
    # one or a few long nodes: runs cross many blocks; 30 + m * IB bases give an interior total of exactly m blocks
    g = synthetic_linear_graph(n_bases, node_len=min(25000, n_bases), seed=5)
    f = DenseKmerFinder(g, 31, only_save_one_node_per_kmer=True, max_variant_nodes=5)
    n_int = _check_split(f)
    assert n_int > 0


@pytest.mark.parametrize("G,S,seed", [(120000, 1500, 9), (300000, 600, 3), (100003, 4000, 21), (64 * 1000 + 7, 300, 2)])
def test_snp_graphs(G, S, seed):
    g = synthetic_snp_graph(G, S, k=31, seed=seed)
    f = DenseKmerFinder(g, 31, only_save_one_node_per_kmer=True, max_variant_nodes=5)
    n_int = _check_split(f)
    _check_against_oracle(g, 31, f)


@pytest.mark.parametrize("k", [5, 15, 31])
def test_dense_sites_force_the_slow_path(k):
    # a site every few bases: hundreds of nodes per block, more than the stage holds, and nodes of k - 1, k, k + 1 bases
    g = synthetic_snp_graph(60000, 60000 // (k + 2), k=k, seed=11)
    f = DenseKmerFinder(g, k, only_save_one_node_per_kmer=True, max_variant_nodes=5)
    _check_split(f)


def test_indel_and_nested_graphs():
    # empty alt nodes and empty linear-ref dummy nodes between the runs; limits at which the reference does not assert
    for g, M in ((synthetic_indel_graph(300000, 3500, k=31, seed=300000 % 97, p_del=0.1, p_ins=0.1), 5),
                 (synthetic_indel_graph(120000, 5000, k=31, seed=120000 % 97, p_del=0.25, p_ins=0.25), 0),
                 (synthetic_nested_graph(200000, 2000, k=31, seed=9, p_nest=0.3), 8)):
        f = DenseKmerFinder(g, 31, only_save_one_node_per_kmer=True, max_variant_nodes=M)
        _check_split(f)


def test_chunked_runs_and_shards():
    g = synthetic_snp_graph(300000, 2500, k=31, seed=13)
    cp = CriticalGraphPaths.from_graph(g, 31)
    n = len(cp)
    cuts = [0] + sorted(np.random.default_rng(1).integers(1, n, size=5).tolist()) + [n]
    f = DenseKmerFinder(g, 31, critical_graph_paths=cp, only_save_one_node_per_kmer=True, max_variant_nodes=5,
                        start_at_critical_path_number=0, stop_at_critical_path_number=n)
    total = 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        f.set_critical_path_range(a, b)       # one finder, its per-finder tables reused chunk after chunk
        _check_split(f)
        total += len(_columns(f.find_flat_on_device(split_layout=True), f)[0])
        _check_against_oracle(g, 31, f, (cp.nodes, cp.offsets), start_at_critical_path_number=a,
                              stop_at_critical_path_number=b)
    full = DenseKmerFinder(g, 31, critical_graph_paths=cp, only_save_one_node_per_kmer=True, max_variant_nodes=5)
    assert total == len(_columns(full.find_flat_on_device(split_layout=True), full)[0])


def test_repeated_steps_into_one_buffer():
    g = synthetic_snp_graph(250000, 2000, k=31, seed=17)
    f = DenseKmerFinder(g, 31, only_save_one_node_per_kmer=True, max_variant_nodes=5)
    first = _columns(f.find_flat_on_device(split_layout=True), f)
    out = None
    for _ in range(3):
        out = f.find_flat_on_device(out)
        again = _columns(out, f)
        for a, b in zip(first, again):
            assert np.array_equal(a, b)
