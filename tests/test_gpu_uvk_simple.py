"""Simple selection on the device (find_kmers_over_variants, the -S True route of make_unique_variant_kmers) against the
reference's stored output and the test-side restatement (tests/spec_uvk_simple.py).  All comparisons are exact."""
import os
import subprocess
import sys

import numpy as np
import pytest

import spec_uvk_simple as spec
import uvk_simple_cases as cases
from oracle import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = cases.load_cases()


class _Pid:
    def __init__(self, base):
        self._base = np.asarray(base, dtype=np.int64)

    def get(self, nodes, offsets):
        return self._base[np.asarray(nodes, dtype=np.int64)] + np.asarray(offsets, dtype=np.int64)


class _V:
    def __init__(self, position, chromosome, line, is_snp):
        self.position, self.chromosome, self.vcf_line_number = position, chromosome, line
        self.type = "SNP" if is_snp else "DELETION"


def _inputs(rows):
    """rows [(POS, chromosome, ref node, alt node, is_snp)], row i on line i."""
    from graph_kmer_index_amd.unique_variant_kmers import VariantArrays, VariantToNodesArrays
    pos, chrom, ref, alt, snp = (np.array([r[i] for r in rows], np.int64) for i in range(5))
    return VariantArrays(pos, chrom, np.arange(len(rows)), snp), VariantToNodesArrays(ref, alt)


def _spec(g, rows, k, m, position_base=None):
    ntro = np.asarray(g.node_to_ref_offset)
    starts = g.chromosome_start_nodes
    return spec.simple_variant_kmers(g, [r[2] for r in rows], [r[3] for r in rows], [r[0] for r in rows], range(len(rows)),
                                     [r[4] for r in rows], k, m, chromosome_offsets=[int(ntro[starts[r[1]]]) for r in rows],
                                     position_base=position_base)


def _same(flat, want):
    got = (flat._hashes, flat._nodes, flat._ref_offsets, flat._allele_frequencies)
    for a, b in zip(got, want):
        assert a.dtype == b.dtype
        assert len(a) == len(b)
        assert np.array_equal(a, b)


def _check(g, rows, k, m, pid=None):
    from graph_kmer_index_amd.unique_variant_kmers import find_kmers_over_variants
    va, v2n = _inputs(rows)
    flat = find_kmers_over_variants(g, v2n, va, k, m, position_id_index=pid)
    want = _spec(g, rows, k, m, None if pid is None else pid._base)
    _same(flat, want)
    return flat


def _graph(chromosomes):
    ns, ed, lin, starts, rows = cases.sites_graph(chromosomes)
    return cases.graph_arrays(ns, ed, lin, starts), rows


def _random(seed, length, n_sites, gap, **kw):
    rng = np.random.default_rng(seed)
    return _graph([cases.random_sites(rng, length, n_sites, gap[0], gap[1] + 1, **kw)])


def _bases(rng, n):
    return "".join(rng.choice(list("acgt"), n))


# ------------------------------------------------------------------ 1. the reference's stored output, API and CLI
def _run_cli(args, tmp_path):
    subprocess.run([sys.executable, "-m", "graph_kmer_index_amd.command_line_interface"] + args, check=True,
                   env=dict(os.environ, PYTHONPATH=ROOT), cwd=str(tmp_path))


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_api_and_cli_equal_the_reference(case, tmp_path):
    from graph_kmer_index_amd.unique_variant_kmers import VariantArrays, VariantToNodesArrays, find_kmers_over_variants
    g = cases.case_graph(case)
    pos, chrom, lines, is_snp, ref, var = cases.case_variants(case)
    want = cases.expected(case)
    k, m = case["k"], case["max_variant_nodes"]
    _same(find_kmers_over_variants(g, VariantToNodesArrays(ref, var), VariantArrays(pos, chrom, lines, is_snp), k, m), want)
    g.to_file(str(tmp_path / "graph.npz"))
    VariantToNodesArrays(ref, var).to_file(str(tmp_path / "v2n.npz"))
    cases.write_vcf(tmp_path / "v.vcf", pos, chrom, is_snp)
    _run_cli(["make_unique_variant_kmers", "-g", "graph.npz", "-V", "v2n.npz", "-k", str(k), "-m", str(m), "-v", "v.vcf",
              "-S", "True", "-c", "7", "-t", "2", "-o", "out"], tmp_path)
    cli = np.load(tmp_path / "out.npz")
    for key, b in zip(("hashes", "nodes", "ref_offsets", "allele_frequencies"), want):
        assert cli[key].dtype == b.dtype and np.array_equal(cli[key], b)


# ------------------------------------------------------------------ 2. forced traversal and the variant limit
@pytest.mark.parametrize("m", [0, 1, 2])
def test_close_sites_at_low_limits(m):
    g, rows = _random(40 + m, 1500, 120, (2, 8))
    pid = _Pid(g.position_id_base() * 3 + 7) if m == 1 else None          # and position ids that are not the default ones
    flat = _check(g, rows, 31, m, pid)
    if m == 2:                                                           # a start before another site: several records per node
        assert np.bincount(flat._nodes.astype(np.int64)).max() > 1


def test_a_variant_that_is_the_first_thing_after_its_start():
    g, rows = _random(44, 6000, 60, (60, 90))
    flat = _check(g, rows, 31, 6)
    assert len(flat._hashes) >= len(rows)


# ------------------------------------------------------------------ 3. node lengths around the window
def _indel_sites(rng):
    """Insertions of 22, 23, 24 and 40 bases and a deletion of 5, 100 bases apart: with k = 31 and a start 8 bases before, the
    k-mer of the 23-base insertion ends on the node's last base, of the 24-base one inside it, of the 22-base one beyond."""
    seq = _bases(rng, 700)
    sites = [(100 * (i + 1), "ins", _bases(rng, n), 0) for i, n in enumerate((22, 23, 24, 40))]
    return seq, sites + [(500, "del", "", 5)]


def test_insertions_around_the_window_length():
    g, rows = _graph([_indel_sites(np.random.default_rng(50))])
    flat = _check(g, rows, 31, 6)
    have = set(flat._nodes.tolist())
    assert all(r[2] in have and r[3] in have for r in rows)              # empty ref dummies and the empty alt node too


@pytest.mark.parametrize("k", [5, 8])
def test_short_k_never_reaches_an_indel_node(k):
    from graph_kmer_index_amd.unique_variant_kmers import find_kmers_over_variants_on_device
    g, rows = _graph([_indel_sites(np.random.default_rng(51))])
    va, v2n = _inputs(rows)
    d = find_kmers_over_variants_on_device(g, v2n, va, k, 6)
    assert d.n == 0
    flat = d.to_flat_kmers()
    d.free()
    _same(flat, _spec(g, rows, k, 6))
    assert flat._hashes.dtype == np.uint64 and len(flat._hashes) == 0


# ------------------------------------------------------------------ 4. where the start falls
def _placement_chromosome(rng):
    """Three SNPs at a, each followed by a deletion at a + 7, a + 8, a + 9: the deletion's start P - 8 is the last base of
    the node before the SNP (two nodes back), the SNP's own one-base node, and offset 0 of the node after it."""
    seq = _bases(rng, 600)
    sites = []
    for i, d in enumerate((7, 8, 9)):
        a = 100 + 150 * i
        sites += [(a, "snp", "acgt"[("acgt".index(seq[a]) + 1) % 4], 1), (a + d, "del", "", 2)]
    return seq, sites


def test_start_placement_on_two_chromosomes():
    rng = np.random.default_rng(60)
    g, rows = _graph([_placement_chromosome(rng), _placement_chromosome(rng)])
    assert {r[1] for r in rows} == {1, 2}
    where = [s[2:] for s in spec.searches(g, [r[2] for r in rows], [r[3] for r in rows], [r[0] for r in rows], range(len(rows)),
                                          [r[4] for r in rows])][:12]
    ref_of = {r[2] for r in rows if r[4]}
    offsets = {(int(g.node_size[n]) - 1 == o, o == 0, n in ref_of) for n, o in where}
    assert (True, False, False) in offsets and (True, True, True) in offsets and (False, True, False) in offsets
    _check(g, rows, 31, 6)


def test_start_before_the_linear_reference_raises():
    from graph_kmer_index_amd.unique_variant_kmers import find_kmers_over_variants
    rng = np.random.default_rng(61)
    g, rows = _graph([(_bases(rng, 300), [(5, "del", "", 2), (100, "del", "", 2)])])
    va, v2n = _inputs(rows[1:] + rows[:1])
    with pytest.raises(ValueError, match="variant 1 .*POS 5"):
        find_kmers_over_variants(g, v2n, va, 31, 6)


# ------------------------------------------------------------------ 5. launch boundaries
def test_130_starts_fill_two_blocks_and_part_of_a_third():
    g, rows = _random(70, 6000, 65, (30, 60))
    assert len(rows) == 65
    _check(g, rows, 31, 6)


def test_three_thousand_variants():
    g, rows = _random(71, 140000, 3000, (10, 60))
    assert len(rows) == 3000
    flat = _check(g, rows, 31, 6)
    assert len(flat._hashes) > 6000


# ------------------------------------------------------------------ 6. the slow path for deep windows
def test_a_run_of_empty_nodes_before_the_variant_takes_the_deep_kernels():
    """40 bases, 60 empty linear-ref nodes in a row, a deletion: the search starts 8 bases before the run and reaches its node
    64 nodes on, past the 48 levels of the product kernel."""
    from graph_kmer_index_amd.graph import GraphArrays
    rng = np.random.default_rng(80)
    ns = {0: _bases(rng, 40)}
    ed, lin = {}, [0]
    for n in range(1, 61):
        ns[n] = ""
        ed[n - 1] = [n]
        lin.append(n)
    ns[61], ns[62], ns[63] = _bases(rng, 2), "", _bases(rng, 60)
    ed[60], ed[61], ed[62] = [61, 62], [63], [63]
    lin += [61, 63]
    g = GraphArrays.from_dicts(ns, ed, lin, chromosome_start_nodes=[0])
    rows = [(40, 1, 61, 62, 0)]
    flat = _check(g, rows, 31, 6)
    assert sorted(flat._nodes.tolist()) == [61, 62]


# ------------------------------------------------------------------ 7. offsets beyond int16 and uint16
def test_offsets_beyond_16_bits():
    rng = np.random.default_rng(90)
    seq = _bases(rng, 70300)
    # a deletion right after a 70 000-base node (node 3), and one base on a SNP-typed site with an empty alt node: the
    # deletion's two searches and the empty node's start beyond offset 65 535 of the long node
    g, rows = _graph([(seq, [(50, "snp", "a" if seq[50] != "a" else "c", 1), (70051, "del", "", 3), (70055, "snp", "", 1)])])
    assert g.node_size[3] == 70000
    # and a line whose ref node is the long node itself, its start inside it: the k-mer ends there at an offset above 32 767
    rows.append((40000, 1, 3, rows[1][3], 0))
    flat = _check(g, rows, 31, 6)
    ids = flat._ref_offsets[flat._nodes == 3].astype(np.int64) - int(g.position_id_base()[3])
    assert len(ids) == 1 and ids[0] == 40000 - 8 - 51 + 30 and ids[0] > 32767
    where = spec.searches(g, [r[2] for r in rows], [r[3] for r in rows], [r[0] for r in rows], range(4), [r[4] for r in rows])
    assert sum(1 for s in where if s[2] == 3 and s[3] > 65535) >= 3


# ------------------------------------------------------------------ 8. the reference's assertion
def test_two_linear_ref_successors_at_the_limit_is_an_assertion_error():
    from graph_kmer_index_amd.graph import GraphArrays
    from graph_kmer_index_amd.unique_variant_kmers import find_kmers_over_variants
    rng = np.random.default_rng(100)
    ns = {0: _bases(rng, 40), 1: "a", 2: "c", 3: _bases(rng, 3), 4: "g", 5: "t", 6: _bases(rng, 50)}
    ed = {0: [1, 2], 1: [3], 2: [3], 3: [4, 5], 4: [6], 5: [6]}
    g = GraphArrays.from_dicts(ns, ed, [0, 1, 2, 3, 4, 6], chromosome_start_nodes=[0])
    rows = [(45, 1, 4, 5, 0)]
    with pytest.raises(oracle.OracleError) as e:
        _spec(g, rows, 31, 0)
    assert e.value.code == 3
    va, v2n = _inputs(rows)
    with pytest.raises(AssertionError):
        find_kmers_over_variants(g, v2n, va, 31, 0)
    _check(g, rows, 31, 1)                                                # below the limit the same search is answered


# ------------------------------------------------------------------ 9. the finder's methods
def test_finder_methods_equal_slices_of_the_batch():
    from graph_kmer_index_amd import CollisionFreeKmerIndex, DenseKmerFinder
    from graph_kmer_index_amd.unique_variant_kmers import UniqueVariantKmersFinder, find_kmers_over_variants
    g, rows = _random(110, 2000, 30, (3, 30))
    va, v2n = _inputs(rows)
    batch = find_kmers_over_variants(g, v2n, va, 31, 6)
    cols = (batch._hashes, batch._nodes, batch._ref_offsets, batch._allele_frequencies)
    f = DenseKmerFinder(g, 31, max_variant_nodes=4)
    f.find()
    finder = UniqueVariantKmersFinder(g, v2n, va, 31, 6, use_dense_kmer_finder=True, position_id_index=_Pid(g.position_id_base()),
                                      kmer_index_with_frequencies=CollisionFreeKmerIndex.from_flat_kmers(f.get_flat_kmers(v="1"),
                                                                                                       modulo=100003))
    at = 0
    kinds = set()
    for i, r in enumerate(rows):
        n_ref = len(_spec(g, [(r[0], r[1], r[2], r[2], r[4])], 31, 6)[0]) // 2
        n_both = len(_spec(g, [r], 31, 6)[0])
        if i % 4 == 0:
            v = _V(r[0], r[1], i, r[4])
            _same(finder.find_kmers_over_variant(v, r[2], r[3]), tuple(c[at:at + n_both] for c in cols))
            _same(finder.find_kmers_over_variant_node(v, r[2]), tuple(c[at:at + n_ref] for c in cols))
            _same(finder.find_kmers_over_variant_node(v, r[3]), tuple(c[at + n_ref:at + n_both] for c in cols))
            kinds.add(r[4])
        at += n_both
    assert at == len(cols[0]) and kinds == {0, 1}
