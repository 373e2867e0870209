"""Simple selection (find_kmers_over_variants) without a GPU: the test-side restatement against the reference's own
output, what the stored cases exercise, and the host layer (VariantArrays types, the -S True route of the CLI)."""
import gzip

import numpy as np
import pytest

import spec_uvk_simple as spec
import uvk_simple_cases as cases

CASES = cases.load_cases()
BY_NAME = {c["name"]: c for c in CASES}
PARAMETERS = {"k31_m6_sparse": (31, 6), "k31_m6_dense": (31, 6), "k15_m6_dense": (15, 6), "k31_m2_dense": (31, 2),
              "k5_m6": (5, 6), "k31_m0_dense": (31, 0), "two_chromosomes": (31, 6), "shared_nodes": (31, 6)}


def _spec(case, **kw):
    g = cases.case_graph(case)
    pos, chrom, lines, is_snp, ref, var = cases.case_variants(case)
    starts = case["graph"]["chromosome_start_nodes"]
    ntro = np.asarray(g.node_to_ref_offset)
    return spec.simple_variant_kmers(g, ref, var, pos, lines, is_snp, case["k"], case["max_variant_nodes"],
                                     chromosome_offsets=[int(ntro[starts[c - 1]]) for c in chrom], **kw)


def test_the_stored_cases_are_the_ones_asked_for():
    assert {c["name"]: (c["k"], c["max_variant_nodes"]) for c in CASES} == PARAMETERS
    for c in CASES:
        assert 0 in c["ref_nodes"]                                    # a skipped line
        assert 0 in c["variants"]["is_snp"] and 1 in c["variants"]["is_snp"]
    assert set(BY_NAME["two_chromosomes"]["variants"]["chromosomes"]) == {1, 2}
    shared = BY_NAME["shared_nodes"]
    assert len(set(shared["ref_nodes"])) < len(shared["ref_nodes"]) - 1
    # insertions (empty ref node) and deletions of several bases (empty alt node)
    seqs = BY_NAME["k31_m6_dense"]["graph"]["node_sequences"]
    dense = BY_NAME["k31_m6_dense"]
    assert any(seqs[str(r)] == "" for r in dense["ref_nodes"] if r)
    assert any(seqs[str(a)] == "" and len(seqs[str(r)]) > 1 for r, a in zip(dense["ref_nodes"], dense["var_nodes"]) if r)


@pytest.mark.parametrize("name", sorted(PARAMETERS))
def test_spec_equals_the_reference(name):
    case = BY_NAME[name]
    got, want = _spec(case), cases.expected(case)
    assert len(want[0]) > 0
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize("name", ["k31_m0_dense", "k31_m2_dense"])
def test_forced_traversal_changes_kmers_in_a_dense_case(name):
    """Without only_follow_nodes the same node gets other k-mers where the path is at the variant limit before it reaches
    the node (with 6 variant nodes allowed that takes six sites inside the 8 bases before one: the M = 6 cases cannot
    show it)."""
    case = BY_NAME[name]
    forced, free = _spec(case), _spec(case, follow=None)
    assert not (len(forced[0]) == len(free[0]) and np.array_equal(forced[0], free[0]))
    assert len(free[0]) < len(forced[0])                                  # nodes behind the limit are not reached


@pytest.mark.parametrize("name", ["k31_m0_dense", "k31_m2_dense"])
def test_one_follow_mask_for_the_batch_is_another_search(name):
    """A mask holding every variant's nodes forces, and waives the limit at, every other site in the window: the paths
    that the limit cuts in the per-node search are walked, and the node gets records the mode does not give it."""
    case = BY_NAME[name]
    every = {n for n in case["ref_nodes"] + case["var_nodes"] if n}
    per_node, masked = _spec(case), _spec(case, follow=every)
    assert len(masked[0]) != len(per_node[0])
    assert len(masked[0]) > len(per_node[0])


def test_k5_leaves_nodes_without_a_record():
    case = BY_NAME["k5_m6"]
    have = set(cases.expected(case)[1].tolist())
    asked = {n for r, a in zip(case["ref_nodes"], case["var_nodes"]) if r and a for n in (r, a)}
    assert len(asked - have) > 10 and have <= asked


# ------------------------------------------------------------------ host layer
class _V:
    def __init__(self, position, chromosome, line, type=None):
        self.position, self.chromosome, self.vcf_line_number, self.type = position, chromosome, line, type


def test_variant_types_from_a_vcf_and_from_objects(tmp_path):
    from graph_kmer_index_amd.unique_variant_kmers import VariantArrays
    text = "##x\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\n1\t10\t.\tA\tC\t.\n1\t20\t.\tAC\tA\t.\n2\t30\t.\tA\tACG\n2\t40\t.\tA\tC,G\n"
    (tmp_path / "v.vcf").write_text(text)
    with gzip.open(tmp_path / "v.vcf.gz", "wt") as f:
        f.write(text)
    for name in ("v.vcf", "v.vcf.gz"):
        va = VariantArrays.from_vcf(str(tmp_path / name))
        assert va.is_snp.dtype == np.int8 and va.is_snp.tolist() == [1, 0, 0, 0]
        assert va.positions.tolist() == [10, 20, 30, 40] and va.chromosomes.tolist() == ["1", "1", "2", "2"]
    (tmp_path / "two.vcf").write_text("1\t10\n1\t20\n")                  # the two-column tolerance stays: type not set
    assert VariantArrays.from_vcf(str(tmp_path / "two.vcf")).is_snp.tolist() == [-1, -1]
    va = VariantArrays.from_objects([_V(5, 1, 0, "SNP"), _V(9, 1, 1, "DELETION"), _V(12, 1, 2, "INSERTION"), _V(15, 1, 3)])
    assert va.is_snp.tolist() == [1, 0, 0, -1]
    assert VariantArrays([1, 2], 1, [0, 1]).is_snp is None               # the three-argument constructor
    with pytest.raises(ValueError):
        VariantArrays([1, 2], 1, [0, 1], [1])


def test_a_variant_without_type_is_the_references_assertion():
    from graph_kmer_index_amd.unique_variant_kmers import (VariantArrays, VariantToNodesArrays, find_kmers_over_variants)
    case = BY_NAME["k31_m6_sparse"]
    g = cases.case_graph(case)
    v2n = VariantToNodesArrays(case["ref_nodes"], case["var_nodes"])
    for variants in ([_V(100, 1, 0, "SNP"), _V(200, 1, 2)], VariantArrays([100], 1, [0])):
        with pytest.raises(AssertionError, match="Variant type must be set"):
            find_kmers_over_variants(g, v2n, variants)


def test_the_constructor_points_at_the_function():
    from graph_kmer_index_amd.unique_variant_kmers import UniqueVariantKmersFinder
    with pytest.raises(NotImplementedError, match="find_kmers_over_variants.*-S True"):
        UniqueVariantKmersFinder(None, None, [], use_dense_kmer_finder=True, use_simple=True)


class _DeviceAsked(Exception):
    pass


def test_cli_simple_route_reaches_the_device_without_a_frequency_source(tmp_path, monkeypatch):
    """-S True needs neither -D nor -i / -I, ignores -N and -H, accepts -c and -t, and gets as far as asking for a device."""
    from graph_kmer_index_amd import _lib, command_line_interface as cli
    from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays
    case = BY_NAME["k31_m6_sparse"]
    pos, chrom, lines, is_snp, ref, var = cases.case_variants(case)
    cases.case_graph(case).to_file(str(tmp_path / "graph.npz"))
    VariantToNodesArrays(ref, var).to_file(str(tmp_path / "v2n.npz"))
    cases.write_vcf(tmp_path / "v.vcf", pos, chrom, is_snp)

    def asked():
        raise _DeviceAsked()
    monkeypatch.setattr(_lib, "require_device", asked)
    args = ["make_unique_variant_kmers", "-g", str(tmp_path / "graph.npz"), "-V", str(tmp_path / "v2n.npz"), "-k", "31",
            "-v", str(tmp_path / "v.vcf"), "-o", str(tmp_path / "out"), "-S", "True"]
    for extra in ([], ["-N", "n", "-H", "h", "-c", "7", "-t", "3"], ["-D", "True"]):
        a = cli.build_parser().parse_args(args + extra)
        assert a.simple
        with pytest.raises(_DeviceAsked):
            a.func(a)
    a = cli.build_parser().parse_args([x for x in args if x not in ("-v", str(tmp_path / "v.vcf"))])
    with pytest.raises(ValueError, match="-v"):
        a.func(a)
