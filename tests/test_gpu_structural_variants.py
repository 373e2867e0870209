"""sample_kmers_from_structural_variants on the device: against the reference's own output
(tests/golden/sv_kmers_reference.json.gz) and, on seeded random graphs, against the test-side restatement
(tests/spec_structural_variants.py).  Everything is compared record for record, in order, with dtypes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import graphgen
import spec_structural_variants as spec

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = spec.load_cases()


def _same(flat, exp):
    got = (flat._hashes, flat._nodes, flat._ref_offsets, flat._allele_frequencies)
    for name, a, b in zip(("hashes", "nodes", "ref_offsets", "allele_frequencies"), got, exp):
        assert a.dtype == b.dtype, name
        assert len(a) == len(b), "%s: %d records, %d expected" % (name, len(a), len(b))
        assert np.array_equal(a, b), name


def _case_index(case):
    from graph_kmer_index_amd import CollisionFreeKmerIndex
    return CollisionFreeKmerIndex.from_flat_kmers(spec.case_index_flat(case), modulo=case["index"]["modulo"])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_fixture_case_equals_reference(case):
    from graph_kmer_index_amd.structural_variants import sample_kmers_from_structural_variants
    from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays
    g, index = spec.case_graph(case), _case_index(case)
    pairs = [tuple(p) for p in case["pairs"]]
    exp = spec.expected(case)
    _same(sample_kmers_from_structural_variants(g, pairs, index, case["k"], case["max_frequency"]), exp)
    arrays = VariantToNodesArrays([p[0] for p in pairs], [p[1] for p in pairs])
    _same(sample_kmers_from_structural_variants(g, arrays, index, case["k"], max_frequency=case["max_frequency"]), exp)


def test_default_max_frequency_is_2():
    from graph_kmer_index_amd.structural_variants import sample_kmers_from_structural_variants
    case = next(c for c in CASES if c["name"] == "max_frequency_2")
    _same(sample_kmers_from_structural_variants(spec.case_graph(case), case["pairs"], _case_index(case), case["k"]),
          spec.expected(case))


def test_device_columns_are_the_merged_layout():
    from graph_kmer_index_amd.structural_variants import sample_kmers_from_structural_variants_on_device
    case = next(c for c in CASES if c["name"] == "long_nodes_sparse")
    d = sample_kmers_from_structural_variants_on_device(spec.case_graph(case), case["pairs"], _case_index(case), case["k"],
                                                        case["max_frequency"])
    h, n, r, af = spec.expected(case)
    assert d.n == len(h)
    flat = d.to_flat_kmers()
    d.free()
    assert (flat._hashes.dtype, flat._nodes.dtype, flat._ref_offsets.dtype, flat._allele_frequencies.dtype) == \
        (np.uint64, np.uint32, np.uint64, np.float32)
    assert np.array_equal(flat._hashes, h) and np.array_equal(flat._nodes, n)
    assert not flat._ref_offsets.any() and np.array_equal(flat._allele_frequencies, af)


# ------------------------------------------------------------------ seeded random graphs
def _graph_with_long_alts(seed, generator, sizes, **kw):
    """A graphgen graph some of whose non-linear nodes are replaced by long inserted sequences of the given sizes; two of
    them share a stretch, so that some windows have frequency 2.  Returns (GraphArrays, (ref, var) pairs)."""
    from graph_kmer_index_amd.graph import GraphArrays
    rng = np.random.default_rng(seed)
    seqs, edges, linear, _ = generator(rng, **kw)
    lin = set(linear)
    alts = [n for n in sorted(seqs) if n not in lin and len(seqs[n]) > 0]
    assert len(alts) >= len(sizes)
    chosen = [alts[i] for i in np.sort(rng.choice(len(alts), size=len(sizes), replace=False))]
    for n, size in zip(chosen, sizes):
        seqs[n] = graphgen._rand_seq(rng, size)
    if len(chosen) >= 2 and min(len(seqs[chosen[0]]), len(seqs[chosen[1]])) >= 120:
        a, b = chosen[0], chosen[1]
        seqs[b] = seqs[b][:20] + seqs[a][10:100] + seqs[b][110:]
    g = GraphArrays.from_dicts(seqs, edges, linear)
    # pairs: (a linear predecessor's other successor or 0, the alt node); every alt twice over the list, some ref == var
    pairs = []
    for n in chosen:
        sib = [s for p, succ in edges.items() if n in succ for s in succ if s != n]
        pairs.append((sib[0] if sib else 0, n))
    pairs += [(chosen[0], chosen[0]), (0, chosen[-1]), (chosen[-1], 0)]
    pairs += [(int(n), 0) for n in linear[:3]]
    return g, pairs


def _own_index(g, k, seed, modulo=1000003):
    """An index of the graph's own k-mers (find(), two thirds of them) plus reverse complements of another part."""
    from graph_kmer_index_amd import CollisionFreeKmerIndex, DenseKmerFinder, FlatKmers
    f = DenseKmerFinder(g, k, max_variant_nodes=100)          # nested variants: no window ends at the variant limit
    f.find()
    flat = f.get_flat_kmers(v="1")
    h = np.asarray(flat._hashes).astype(np.uint64)
    keep = h % np.uint64(3) != 0
    part = FlatKmers(h[keep], np.asarray(flat._nodes)[keep], np.asarray(flat._ref_offsets)[keep],
                     np.asarray(flat._allele_frequencies)[keep])
    rc_of = h % np.uint64(5) == 1
    rc = FlatKmers(h[rc_of], np.asarray(flat._nodes)[rc_of], np.asarray(flat._ref_offsets)[rc_of],
                   np.asarray(flat._allele_frequencies)[rc_of]).get_reverse_complement_flat_kmers(k)
    return CollisionFreeKmerIndex.from_flat_kmers(FlatKmers.from_multiple_flat_kmers([part, rc]), modulo=modulo)


def _random_case(seed, generator, sizes, k, max_frequencies, **kw):
    from graph_kmer_index_amd.structural_variants import sample_kmers_from_structural_variants
    g, pairs = _graph_with_long_alts(seed, generator, sizes, **kw)
    index = _own_index(g, k, seed)
    table = spec.FrequencyTable.from_index(index)
    total = 0
    for mf in max_frequencies:
        h, n, r = spec.sample_kmers(g, pairs, table, k, mf)
        got = sample_kmers_from_structural_variants(g, pairs, index, k, mf)
        _same(got, (h, n, r, np.ones(len(h), np.float32)))
        assert got._ref_offsets.dtype == np.uint32 and not got._ref_offsets.any()       # the reference stores no position here
        total += len(h)
    assert total > 0
    return g, got


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("k", [31, 15])
def test_random_bubble_graph_matches_spec(seed, k):
    _random_case(seed, graphgen.random_bubble_graph, [40, 36, 37, 100, 700, 5000], k, (1, 2, 3), n_var=40, p_indel=0.6)


@pytest.mark.parametrize("seed", [4, 5])
def test_random_nested_graph_matches_spec(seed):
    _random_case(seed, graphgen.nested_bubble_graph, [45, 64 + 30, 4096 + 30, 4097 + 30, 12000], 31, (2, 5), n_var=30)


def test_random_graph_with_a_200000_base_node_matches_spec():
    g, got = _random_case(6, graphgen.random_bubble_graph, [200000, 60000, 40, 9000], 31, (1, 2), n_var=30, p_indel=0.6)
    # a sampled window that lies beyond offset 65 536 of the 200 000-base node: its hash read from the sequence there
    node = int(np.argmax(g.node_size))
    assert g.node_size[node] == 200000
    s = g.seq[g.seq_start[node] + 65536:g.seq_start[node + 1]].astype(np.uint64)
    far = sum(s[i:len(s) - 30 + i] << np.uint64(2 * i) for i in range(31))
    assert np.count_nonzero(np.isin(got._hashes[got._nodes == node], far)) > 0
    _random_case(7, graphgen.random_bubble_graph, [150000, 50], 23, (2,), n_var=20, p_indel=0.6)


# ------------------------------------------------------------------ refusals
def test_refused_arguments():
    from graph_kmer_index_amd import _lib
    from graph_kmer_index_amd.device_graph import DeviceGraph
    from graph_kmer_index_amd.structural_variants import sample_kmers_from_structural_variants
    case = next(c for c in CASES if c["name"] == "greedy_rule")
    g, index = spec.case_graph(case), _case_index(case)
    pairs = case["pairs"]

    class Counter:
        def get_frequency(self, kmer):
            return 0

    with pytest.raises(NotImplementedError, match="CollisionFreeKmerIndex"):
        sample_kmers_from_structural_variants(g, pairs, Counter(), 31)
    for k in (0, 32):
        with pytest.raises(ValueError, match="k must be in 1..31"):
            sample_kmers_from_structural_variants(g, pairs, index, k)
    with pytest.raises(ValueError, match="max_frequency"):
        sample_kmers_from_structural_variants(g, pairs, index, 31, max_frequency=-1)
    with pytest.raises(ValueError, match="names node"):
        sample_kmers_from_structural_variants(g, [(3, g.n_nodes)], index, 31)
    # the C entry point refuses the same values
    lib = _lib.load()
    dg = DeviceGraph.of(g)
    view = index._device_index().view()
    n_rec, plan = _lib._I64(0), _lib.C.c_void_p()

    def count(d_cand, n, k, mf):
        return lib.gki_sv_sample_count(dg.handle, _lib.C.byref(view), d_cand.ptr, n, k, mf, None, _lib.C.byref(n_rec),
                                       _lib.C.byref(plan), None)

    good = _lib.DeviceArray.from_host(np.array([3, 5], dtype=np.int32))
    for k, mf in ((0, 2), (32, 2), (31, -1)):
        assert count(good, 2, k, mf) == 2 and not plan.value                 # GKI_ERR_BAD_ARG
    for node in (g.n_nodes, -1):
        bad = _lib.DeviceArray.from_host(np.array([3, node], dtype=np.int32))
        assert count(bad, 2, 31, 2) == 2 and not plan.value
        assert b"candidate 1" in lib.gki_last_error()
    assert count(good, 2, 31, 2) == 0 and plan.value and n_rec.value == len(case["expected"]["hashes"])
    assert lib.gki_sv_sample_destroy(plan) == 0


# ------------------------------------------------------------------ command line
def _run_cli(args, tmp_path, check=True):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "graph_kmer_index_amd.command_line_interface"] + args, check=check, env=env,
                          cwd=str(tmp_path), stderr=subprocess.PIPE, text=True)


def test_cli_round_trip_sample_merge_make_from_flat(tmp_path):
    from graph_kmer_index_amd import CollisionFreeKmerIndex
    from graph_kmer_index_amd.graph import synthetic_snp_graph
    from graph_kmer_index_amd.structural_variants import sample_kmers_from_structural_variants
    from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays
    from uvk_cases import bubble_variants
    g = synthetic_snp_graph(5000, 60, k=31, seed=7)
    refs, alts, pos = bubble_variants(g, 31)
    index = _own_index(g, 31, 7, modulo=100003)
    g.to_file(str(tmp_path / "graph.npz"))
    index.to_file(str(tmp_path / "index"))
    VariantToNodesArrays(refs, alts).to_file(str(tmp_path / "v2n.npz"))
    # the big nodes of this graph are the segments between its sites: they stand for the structural variants' nodes
    big = np.nonzero(g.node_size > 31 + 5)[0]
    assert len(big) > 10
    sv_pairs = VariantToNodesArrays(big, np.concatenate([big[1:], [0]]))
    sv_pairs.to_file(str(tmp_path / "sv_v2n.npz"))
    with open(tmp_path / "v.vcf", "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n")
        for p in pos:
            f.write("1\t%d\t.\tA\tC\n" % p)
    _run_cli(["make_unique_variant_kmers", "-g", "graph.npz", "-V", "v2n.npz", "-k", "31", "-i", "index.npz", "-D", "True",
              "-v", "v.vcf", "-o", "uvk"], tmp_path)
    _run_cli(["sample_kmers_from_structural_variants", "-g", "graph.npz", "-V", "sv_v2n.npz", "-k", "31", "-i", "index.npz",
              "-t", "4", "-o", "sv"], tmp_path)
    cli = np.load(tmp_path / "sv.npz")
    api = sample_kmers_from_structural_variants(g, sv_pairs, index, 31)
    assert len(api._hashes) > 0
    assert sorted(cli.files) == ["allele_frequencies", "hashes", "nodes", "ref_offsets"]
    for key, a in (("hashes", api._hashes), ("nodes", api._nodes), ("ref_offsets", api._ref_offsets),
                   ("allele_frequencies", api._allele_frequencies)):
        assert cli[key].dtype == a.dtype and np.array_equal(cli[key], a)
    assert cli["ref_offsets"].dtype == np.uint32
    exp = spec.sample_kmers(g, np.stack([sv_pairs.ref_nodes, sv_pairs.var_nodes], axis=1),
                            spec.FrequencyTable.from_index(index), 31, 2)
    assert np.array_equal(cli["hashes"], exp[0]) and np.array_equal(cli["nodes"], exp[1])
    _run_cli(["merge_flat_kmers", "-f", "uvk.npz,sv.npz", "-o", "merged"], tmp_path)
    merged, uvk = np.load(tmp_path / "merged.npz"), np.load(tmp_path / "uvk.npz")
    assert merged["ref_offsets"].dtype == np.uint64                       # uint64 + uint32 by NumPy promotion
    assert len(merged["hashes"]) == len(uvk["hashes"]) + len(cli["hashes"])
    assert np.array_equal(merged["hashes"][len(uvk["hashes"]):], cli["hashes"])
    _run_cli(["make_from_flat", "-f", "merged.npz", "-o", "variant_index", "-m", "100003"], tmp_path)
    built = CollisionFreeKmerIndex.from_file(str(tmp_path / "variant_index"))
    for i in (0, len(cli["hashes"]) // 2, len(cli["hashes"]) - 1):
        nodes = built.get_nodes(int(cli["hashes"][i]), max_hits=1000)
        assert nodes is not None and int(cli["nodes"][i]) in [int(x) for x in nodes]
    # -I is refused, -i is required
    r = _run_cli(["sample_kmers_from_structural_variants", "-g", "graph.npz", "-V", "sv_v2n.npz", "-k", "31", "-I", "counter",
                  "-o", "sv2"], tmp_path, check=False)
    assert r.returncode != 0 and "-I is not supported" in r.stderr
    r = _run_cli(["sample_kmers_from_structural_variants", "-g", "graph.npz", "-V", "sv_v2n.npz", "-k", "31", "-o", "sv2"],
                 tmp_path, check=False)
    assert r.returncode != 0 and "-i" in r.stderr
