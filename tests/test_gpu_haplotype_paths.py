"""Haplotype paths on the device (graph_kmer_index_amd.haplotype_paths, csrc/gki_haplotype_paths.hip) against the spec
(tests/spec_haplotype_paths.py) on the cases of tests/haplotype_path_cases.py: sequences, bounds, alt nodes, node counts,
the three sub-commands from files, and what stays on the device after close()."""
import functools

import numpy as np
import pytest

import spec_haplotype_paths as spec
from graph_build_cases import mixed_lines, line, random_reference
from haplotype_path_cases import CASE_NAMES, COUNT_CASES, case
from graph_kmer_index_amd import CollisionFreeKmerIndex, DenseKmerFinder, _lib
from graph_kmer_index_amd.haplotype_paths import AltPlane, HaplotypePaths, HaplotypeToNodes
from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays
from graph_kmer_index_amd.vcf_files import HaplotypeMatrix

pytestmark = pytest.mark.gpu
MODULO = 2_000_003


def starts_of(graph):
    return [graph.chromosome_start_nodes[c] for c in sorted(graph.chromosome_start_nodes)]


def matrix_of(c):
    return HaplotypeMatrix(c.codes, np.ones(len(c.codes), np.uint8), c.n_slots, 1)


def paths_of(c):
    return HaplotypePaths(c.graph, VariantToNodesArrays(c.ref_nodes, c.var_nodes), matrix_of(c))


@functools.lru_cache(maxsize=None)
def spelled(name, slot):
    c = case(name)
    return spec.spell(c.graph, c.ref_nodes, c.var_nodes, c.codes, slot, starts_of(c.graph))


@pytest.mark.parametrize("name", CASE_NAMES)
def test_sequences_and_alt_nodes_equal_the_spec(name, tmp_path):
    c = case(name)
    with paths_of(c) as paths:
        for slot in range(c.n_slots):
            want = spelled(name, slot)
            ref = paths.sequence(slot)
            try:
                assert ref.names == [str(i + 1) for i in range(len(want))]
                assert ref.bounds.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist(), (name, slot)
                assert ref.letters.n == ref.bounds[-1]
                got = ref.to_host()
            finally:
                ref.free()
            for g, w in zip(got, want):
                assert np.array_equal(g, w), (name, slot, int(np.argmax(g != w)) if len(g) == len(w) else -1)
        table = paths.alt_nodes()
        for slot in (-1, c.n_slots):
            with pytest.raises(IndexError):
                paths.sequence(slot)
    assert table.n_slots == c.n_slots and table.start[0] == 0 and table.start[-1] == len(table.nodes)
    for slot in range(c.n_slots):
        assert np.array_equal(table.nodes_of(slot), spec.alt_nodes(c.var_nodes, c.codes, slot)), (name, slot)
    table.to_file(str(tmp_path / "h2n"))
    back = HaplotypeToNodes.from_file(str(tmp_path / "h2n"))
    assert np.array_equal(back.start, table.start) and np.array_equal(back.nodes, table.nodes)
    assert back.start.dtype == np.int64 and back.nodes.dtype == np.uint32
    assert (back.n_samples, back.ploidy, back.sample_names) == (c.n_slots, 1, None)


def test_a_plane_on_the_device_with_set_tail_bits():
    """The plane's bits at and beyond the line count are masked by kept_bits, not relied on."""
    c = case("lines_65")
    v, h = len(c.var_nodes), c.n_slots
    words = (v + 63) // 64
    plane = np.zeros((h, words), dtype=np.uint64)
    for slot in range(h):
        for line_no in np.flatnonzero(c.codes[:, slot] == 1):
            plane[slot, line_no >> 6] |= np.uint64(1) << np.uint64(line_no & 63)
    plane[:, -1] |= ~((np.uint64(1) << np.uint64(v & 63)) - np.uint64(1))
    with _lib.DeviceScope() as s:
        alt_bits = s.on_device(plane.reshape(-1), np.uint64)
        with HaplotypePaths(c.graph, VariantToNodesArrays(c.ref_nodes, c.var_nodes), AltPlane(alt_bits, v, h)) as paths:
            table = paths.alt_nodes()
            ref = s.keep(paths.sequence(1))
            assert np.array_equal(ref.to_host()[0], spelled("lines_65", 1)[0])
    for slot in range(h):
        assert np.array_equal(table.nodes_of(slot), spec.alt_nodes(c.var_nodes, c.codes, slot)), slot


@functools.lru_cache(maxsize=None)
def index_of(name, k):
    """The case's variant index by the package's own route: find() into from_flat_kmers."""
    finder = DenseKmerFinder(case(name).graph, k, max_variant_nodes=4)
    finder.find()
    return CollisionFreeKmerIndex.from_flat_kmers(finder.get_flat_kmers(v="1"), modulo=MODULO)


@pytest.mark.parametrize("k", [5, 31])
@pytest.mark.parametrize("name", COUNT_CASES)
def test_node_counts_equal_the_spec_and_map_reads(name, k):
    c = case(name)
    index, n_nodes = index_of(name, k), c.graph.n_nodes
    with paths_of(c) as paths:
        # at k = 5 every k-mer has hundreds of hits on a few hundred nodes, so a slot is a fraction of a second of atomics:
        # two slots with reverse complements, one of them without
        for rc, slots in ((True, [4, 1]), (False, [4])):
            got = paths.node_counts(slots, index, k, n_nodes, include_reverse_complement=rc)
            assert got.shape == (len(slots), n_nodes) and got.dtype == np.uint32
            for row, slot in zip(got, slots):
                strings = spelled(name, slot)
                want = spec.node_counts(strings, index, k, n_nodes, rc)
                assert want.sum() > 0
                assert np.array_equal(row, want), (name, k, slot, rc)
                mapped = index.map_reads([s.tobytes().decode() for s in strings], k, n_nodes, include_reverse_complement=rc)
                assert np.array_equal(row, mapped), (name, k, slot, rc)
            if rc:
                whole = got
        # passes that end inside chromosomes
        assert np.array_equal(paths.node_counts([4, 1], index, k, n_nodes, chunk_kmers=1000), whole)
        assert np.array_equal(paths.node_counts([1], index, k)[0], whole[1][:int(index.max_node_id()) + 1])


def live_allocations():
    mallocs, frees = _lib.pool_stats()[:2]
    return mallocs - frees


def test_close_gives_everything_back():
    c = case("mixed_random_two_chromosomes")
    index = index_of("mixed_random_two_chromosomes", 5)
    index._device_index().probe_table()
    with paths_of(c) as warm:                              # whatever the first use of a route parks stays out of the count
        warm.sequence(0).free()
        warm.alt_nodes()
        warm.node_counts([0], index, 5, c.graph.n_nodes)
    _lib.check(_lib.load().gki_trim())
    before = live_allocations()
    paths = paths_of(c)
    paths.sequence(3).free()
    paths.alt_nodes()
    paths.node_counts([2, 3], index, 5, c.graph.n_nodes, chunk_kmers=777)
    with pytest.raises(IndexError):
        paths.node_counts([0, 5], index, 5, c.graph.n_nodes)
    paths.close()
    paths.close()
    with pytest.raises(ValueError, match="closed"):
        paths.sequence(0)
    _lib.check(_lib.load().gki_trim())
    assert live_allocations() == before


def test_from_files_through_the_three_sub_commands(tmp_path):
    from graph_kmer_index_amd.command_line_interface import main
    from graph_kmer_index_amd.fasta_files import parse_fasta_on_device
    from graph_kmer_index_amd.graph_files import build_graph_from_files
    from graph_kmer_index_amd.vcf_files import haplotype_matrix_from_file
    a, b = random_reference(3001, 31, p_n=0.01, p_lower=0.1), random_reference(1500, 32)
    rng = np.random.default_rng(33)
    forms = [b"0|0", b"0|1", b"1|0", b"1|1", b"1|2", b".|1", b"0|."]
    lines = []
    for chrom, ref, n, seed in (("chrA", a, 90, 34), ("chrB", b, 40, 35)):
        for raw in mixed_lines(chrom, ref, n, seed):
            f = raw.rstrip(b"\n").split(b"\t")
            gts = [forms[i] for i in rng.integers(0, len(forms), size=3)]
            lines.append(line(chrom, int(f[1]), f[3], f[4], tail=b"\t.\tPASS\t.\tGT\t" + b"\t".join(gts)))
    header = b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS1\tS2\tS3\n"
    fasta, vcf = str(tmp_path / "ref.fa"), str(tmp_path / "v.vcf")
    with open(fasta, "wb") as f:
        f.write(b">chrA\n" + a + b"\n>chrB\n" + b + b"\n")
    with open(vcf, "wb") as f:
        f.write(header + b"".join(lines))
    built = build_graph_from_files(fasta, vcf)
    matrix = haplotype_matrix_from_file(vcf)
    assert (matrix.n_samples, matrix.ploidy, matrix.n_variants) == (3, 2, len(lines)) and matrix.sample_names == ["S1", "S2", "S3"]
    assert {0, 1, 2, 3} <= set(np.unique(matrix.codes).tolist()) and np.count_nonzero(built.variant_to_nodes.var_nodes) > 60
    g, v2n = built.graph, built.variant_to_nodes
    files = {n: str(tmp_path / n) for n in ("graph", "v2n", "matrix", "index", "h2n", "counts")}
    g.to_file(files["graph"]), v2n.to_file(files["v2n"]), matrix.to_file(files["matrix"])
    finder = DenseKmerFinder(g, 31, max_variant_nodes=4)
    finder.find()
    index = CollisionFreeKmerIndex.from_flat_kmers(finder.get_flat_kmers(v="1"), modulo=MODULO)
    index.to_file(files["index"])
    common = ["-g", files["graph"] + ".npz", "-V", files["v2n"], "-m", files["matrix"]]

    assert main(["make_haplotype_to_nodes"] + common + ["-o", files["h2n"]]) == 0
    table = HaplotypeToNodes.from_file(files["h2n"])
    assert (table.n_samples, table.ploidy, table.sample_names, table.n_slots) == (3, 2, ["S1", "S2", "S3"], 6)
    for slot in range(6):
        assert np.array_equal(table.nodes_of(slot), spec.alt_nodes(v2n.var_nodes, matrix.codes, slot)), slot

    want = {slot: spec.spell(g, v2n.ref_nodes, v2n.var_nodes, matrix.codes, slot, starts_of(g)) for slot in (1, 4)}
    for slot in (1, 4):
        out = str(tmp_path / ("h%d.fa" % slot))
        assert main(["spell_haplotype"] + common + ["-s", str(slot), "-o", out]) == 0
        text = open(out, "rb").read()
        assert max(len(x) for x in text.split(b"\n")) == 60
        back = parse_fasta_on_device(np.frombuffer(text, dtype=np.uint8))
        try:
            assert back.names == ["1", "2"]
            for got, w in zip(back.to_host(), want[slot]):
                assert np.array_equal(got, w), slot
        finally:
            back.free()

    assert main(["haplotype_node_counts"] + common + ["-i", files["index"], "-k", "31", "-s", "4,1", "-o", files["counts"]]) == 0
    counts = np.load(files["counts"] + ".npy")
    n_nodes = int(index.max_node_id()) + 1
    assert counts.shape == (2, n_nodes) and counts.dtype == np.uint32
    for row, slot in zip(counts, (4, 1)):
        assert np.array_equal(row, spec.node_counts(want[slot], index, 31, n_nodes)), slot
