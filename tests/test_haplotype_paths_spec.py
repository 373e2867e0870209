"""The haplotype-path spec (tests/spec_haplotype_paths.py) and the host side of graph_kmer_index_amd.haplotype_paths, checked
without a device: the spec's walk along the edges equals the gather the kernels implement, evaluated in NumPy from the
plan's own host arrays, and equals the reference text edited directly; the plan refuses what the rules refuse; the command
line knows the three sub-commands."""
import numpy as np
import pytest

import spec_graph_build
import spec_haplotype_paths as spec
from haplotype_path_cases import CASE_NAMES, TILE, case
from graph_kmer_index_amd import haplotype_paths as hp
from graph_kmer_index_amd.command_line_interface import build_parser
from graph_kmer_index_amd.graph import synthetic_nested_graph, synthetic_snp_graph
from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays
from graph_kmer_index_amd.vcf_files import HaplotypeMatrix


def starts_of(graph):
    return [graph.chromosome_start_nodes[c] for c in sorted(graph.chromosome_start_nodes)]


def gather(plan, codes, slot):
    """(letters, bounds, cut) by the formula of DESIGN.md 4.19, from the plan's host arrays."""
    alt = codes[plan["kept_line"], slot] == 1 if len(plan["kept_line"]) else np.zeros(0, bool)
    drop_len = np.where(alt, plan["ref_size"], plan["alt_size"]).astype(np.int64)
    drop_start = np.where(alt, plan["ref_start"], plan["alt_start"])
    before = np.concatenate([[0], np.cumsum(drop_len)]).astype(np.int64)
    cut = drop_start - before[:-1]
    n_out = len(plan["seq"]) - before[-1]
    p = np.arange(n_out, dtype=np.int64)
    letters = spec.LETTERS[plan["seq"][p + before[np.searchsorted(cut, p, side="right")]]]
    bounds = plan["chrom_seq_start"] - before[plan["chrom_first_kept"]]
    return letters, bounds, cut


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_walk_equals_the_gather(name):
    c = case(name)
    plan = hp.bubble_chain_plan(c.graph, VariantToNodesArrays(c.ref_nodes, c.var_nodes))
    assert plan["n_lines"] == len(c.var_nodes) and len(plan["kept_line"]) == int(np.sum(c.build.line_status == 0))
    for slot in range(c.n_slots):
        walked = spec.spell(c.graph, c.ref_nodes, c.var_nodes, c.codes, slot, starts_of(c.graph))
        letters, bounds, cut = gather(plan, c.codes, slot)
        assert np.all(np.diff(cut) >= 0), (name, slot)
        assert np.array_equal(np.concatenate(walked), letters), (name, slot)
        assert bounds.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in walked])]).tolist(), (name, slot)


def edited_reference(c, slot):
    """The haplotype's letters per chromosome from the text alone: every kept line at which the slot takes the alt allele
    replaces [lo, hi) of the reference by the alt allele, under the site rule of tests/spec_graph_build.py."""
    names, c0, at = list(c.reference), {}, 0
    for n in names:
        c0[n] = at
        at += len(c.reference[n])
    edits = {n: [] for n in names}
    for v, f in enumerate(spec_graph_build.data_lines(c.text)):
        if c.build.line_status[v] != 0 or c.codes[v][slot] != 1:
            continue
        ref, alt, pos = f[3], f[4], int(f[1])
        if len(ref) != len(alt) and spec_graph_build.upper(ref[0]) == spec_graph_build.upper(alt[0]):
            ref, alt, pos = ref[1:], alt[1:], pos + 1
        edits[f[0].decode()].append((pos - 1, len(ref), alt))
    out = []
    for n in names:
        text, p = b"", 0
        for lo, ref_len, alt in edits[n]:
            text += bytes(c.reference[n][p:lo]) + alt
            p = lo + ref_len
        text += bytes(c.reference[n][p:])
        out.append(spec.LETTERS[np.array([spec_graph_build.CODE.get(x, 0) for x in text], dtype=np.int64)])
    return out


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_walk_equals_the_edited_reference(name):
    c = case(name)
    for slot in range(c.n_slots):
        walked = spec.spell(c.graph, c.ref_nodes, c.var_nodes, c.codes, slot, starts_of(c.graph))
        want = edited_reference(c, slot)
        assert len(walked) == len(want)
        for w, e in zip(walked, want):
            assert np.array_equal(w, e), (name, slot)


def test_alt_nodes_of_the_spec():
    c = case("mixed_random_two_chromosomes")
    kept = c.var_nodes[c.var_nodes != 0]
    assert spec.alt_nodes(c.var_nodes, c.codes, 0).tolist() == []
    assert spec.alt_nodes(c.var_nodes, c.codes, 1).tolist() == kept.tolist()
    some = spec.alt_nodes(c.var_nodes, c.codes, 4)
    assert 0 < len(some) < len(kept) and set(np.unique(c.codes[c.var_nodes != 0, 4]).tolist()) == {0, 1, 2, 3}


def test_node_counts_of_the_spec_equal_the_read_side_reference():
    """spec.node_counts looks every distinct hash up once; hash by hash, tests/read_side_ref.py gives the same."""
    import read_side_ref

    class Index:
        pass
    c = case("mixed_random_two_chromosomes")
    strings = spec.spell(c.graph, c.ref_nodes, c.var_nodes, c.codes, 2, starts_of(c.graph))
    letters = np.concatenate(strings)
    read_start = np.array([0, len(strings[0]), len(letters)], dtype=np.int64)
    rng = np.random.default_rng(41)
    for k in (5, 31):
        forward, _ = read_side_ref.hash_reads_ref(letters, read_start, k, 0)
        index = Index()
        index._kmers = np.concatenate([forward[::3], forward[::7]])
        index._nodes = rng.integers(1, 50, size=len(index._kmers)).astype(np.uint32)
        index._modulo = 2003
        for rc in (True, False):
            want = np.zeros(40, dtype=np.int64)
            for strand in (0, 1) if rc else (0,):
                hashes, _ = read_side_ref.hash_reads_ref(letters, read_start, k, strand)
                want += read_side_ref.count_nodes_ref(spec.index_arrays(index), hashes, 2 ** 62, 40)[0]
            assert want.sum() > 0 and np.array_equal(spec.node_counts(strings, index, k, 40, rc), want), (k, rc)


def test_census_of_the_cases():
    """The shapes the gather can go wrong at are among the cases."""
    lines = {len(case(n).var_nodes) for n in CASE_NAMES}
    assert {0, 63, 64, 65, 129, 2047, 2048, 2049} <= lines
    lengths, in_block, zero_drops, long_drop, tile_cuts, offsets = set(), 0, 0, 0, set(), set()
    for name in CASE_NAMES:
        c = case(name)
        plan = hp.bubble_chain_plan(c.graph, VariantToNodesArrays(c.ref_nodes, c.var_nodes))
        for slot in range(c.n_slots):
            letters, bounds, cut = gather(plan, c.codes, slot)
            lengths.add(len(letters))
            inside = cut[(cut > 0) & (cut < len(letters))]
            in_block = max(in_block, int(np.max(np.bincount(inside // 16))) if len(inside) else 0)
            alt = c.codes[plan["kept_line"], slot] == 1
            drops = np.where(alt, plan["ref_size"], plan["alt_size"])
            zero_drops += int(np.sum(drops == 0))
            long_drop = max(long_drop, int(drops.max()) if len(drops) else 0)
            if len(letters) > 2 * TILE:
                tile_cuts.update((inside % TILE).tolist())
            if name == "snps_17_apart":
                offsets.update((inside % 16).tolist())
            if len(bounds) > 2:
                assert np.all(np.diff(bounds) > 0)
    assert any(n < 16 for n in lengths) and 16 in lengths and any(n % 16 for n in lengths if n > 16)
    assert in_block >= 3 and zero_drops > 0 and long_drop > TILE
    assert {0, TILE - 1} <= tile_cuts and offsets == set(range(16))


def small_inputs():
    g = synthetic_snp_graph(2000, 20, 31, 5)
    alts = np.flatnonzero(g.is_ref == 0)
    return g, alts - 1, alts


def test_a_matrix_of_another_length_is_refused():
    g, ref, var = small_inputs()
    matrix = HaplotypeMatrix(np.zeros((len(var) + 1, 2), np.uint8), np.ones(len(var) + 1, np.uint8), 1, 2)
    with pytest.raises(ValueError, match="%d data lines, variant-to-nodes has %d" % (len(var) + 1, len(var))):
        hp.HaplotypePaths(g, VariantToNodesArrays(ref, var), matrix)


def test_a_nested_graph_is_refused():
    g = synthetic_nested_graph(3000, 30, 31, 7, p_nest=0.5)
    alt_in = np.flatnonzero((g.is_ref == 0) & (np.concatenate([[1], g.is_ref[:-1]]) == 1))
    with pytest.raises(ValueError, match="not a bubble chain: node %d " % (alt_in[np.argmax(g.is_ref[alt_in + 1] == 0)] + 1)):
        hp.bubble_chain_plan(g, VariantToNodesArrays(alt_in - 1, alt_in))


def test_var_not_ref_plus_one_is_refused():
    g, ref, var = small_inputs()
    ref = ref.copy()
    ref[3] -= 1
    with pytest.raises(ValueError, match="data line 3 .* var_nodes == ref_nodes \\+ 1"):
        hp.bubble_chain_plan(g, VariantToNodesArrays(ref, var))


def test_lines_out_of_order_are_refused():
    g, ref, var = small_inputs()
    order = np.arange(len(var))
    order[[4, 5]] = [5, 4]
    with pytest.raises(ValueError, match="data line 5 .* does not ascend"):
        hp.bubble_chain_plan(g, VariantToNodesArrays(ref[order], var[order]))


def test_a_good_graph_passes_and_lines_without_nodes_are_not_kept():
    g, ref, var = small_inputs()
    ref, var = np.insert(ref, 2, 0), np.insert(var, 2, 0)
    plan = hp.bubble_chain_plan(g, VariantToNodesArrays(ref, var))
    assert plan["kept_line"].tolist() == [v for v in range(len(var)) if v != 2]
    assert plan["kept_bits"].tolist() == [((1 << len(var)) - 1) & ~4]


def test_a_slot_out_of_range_is_an_index_error():
    assert hp.check_slot(4, 5) == 4
    for slot in (-1, 5):
        with pytest.raises(IndexError):
            hp.check_slot(slot, 5)
    with pytest.raises(IndexError):
        hp.HaplotypeToNodes([0, 1, 1], [7]).nodes_of(2)


def test_passes_never_cross_a_record_and_hold_at_most_chunk_kmers():
    bounds = np.array([0, 40, 44, 100])
    assert hp.kmer_passes(bounds, 5, 1 << 28) == [([0, 44], [36, 52])]
    passes = hp.kmer_passes(bounds, 5, 30)
    assert [sum(n) for _, n in passes] == [30, 30, 28]
    starts = [a + j for first, count in passes for a, n in zip(first, count) for j in range(n)]
    assert starts == list(range(0, 36)) + list(range(44, 96))


def test_the_fasta_writer_wraps_at_60(tmp_path):
    records = [spec.LETTERS[np.arange(n) % 4] for n in (0, 59, 60, 61, 120)]
    hp.write_fasta(str(tmp_path / "h.fa"), ["1", "2", "3", "4", "5"], records)
    lines = open(str(tmp_path / "h.fa")).read().split("\n")
    assert lines[-1] == "" and [x for x in lines if x.startswith(">")] == [">1", ">2", ">3", ">4", ">5"]
    body, name = {}, None
    for x in lines[:-1]:
        if x.startswith(">"):
            name = x[1:]
            body[name] = []
        else:
            body[name].append(x)
    assert [[len(x) for x in body[n]] for n in "12345"] == [[], [59], [60], [60, 1], [60, 60]]
    assert "".join(body["4"]) == records[3].tobytes().decode()


def test_the_parser_knows_the_three_sub_commands():
    p = build_parser()
    a = p.parse_args(["make_haplotype_to_nodes", "-g", "g", "-V", "v", "-m", "m", "-o", "o"])
    assert (a.graph, a.variant_to_nodes, a.haplotype_matrix, a.out_file_name, a.func.__name__) == ("g", "v", "m", "o", "make_haplotype_to_nodes")
    a = p.parse_args(["spell_haplotype", "-g", "g", "-V", "v", "-m", "m", "-s", "3", "-o", "o.fa"])
    assert (a.slot, a.out_file_name, a.func.__name__) == (3, "o.fa", "spell_haplotype")
    a = p.parse_args(["haplotype_node_counts", "-g", "g", "-V", "v", "-m", "m", "-i", "i", "-s", "0,1,5"])
    assert (a.kmer_index, a.kmer_size, a.slots, a.out_file_name, a.func.__name__) == ("i", 31, "0,1,5", None, "haplotype_node_counts")
    a = p.parse_args(["haplotype_node_counts", "-g", "g", "-V", "v", "-m", "m", "-i", "i", "-k", "5", "-s", "2", "-o", "c.npy"])
    assert (a.kmer_size, a.out_file_name) == (5, "c.npy")
