"""The spec of the node counts by difference and of the count model (tests/spec_haplotype_count_model.py) and the host side
of graph_kmer_index_amd.haplotype_paths, checked without a device: the rule's segments are exactly the dirty windows, each
once; base - removed + added equals counting every window of the spelled strings; the formula the kernels evaluate from the
plan's arrays gives the spec's segments; the model on hand-worked examples; the host argument checks."""
import numpy as np
import pytest

import spec_haplotype_count_model as spec
import spec_haplotype_paths
from haplotype_count_model_cases import CASE_NAMES, KS, case, model_case
from graph_kmer_index_amd import haplotype_paths as hp
from graph_kmer_index_amd.command_line_interface import build_parser
from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays


def both_walks(c, slot):
    """((bounds, intervals) along the all-ref path, (bounds, intervals) along the slot) of the slot's taken lines."""
    return tuple(spec.walk(c.graph, c.ref_nodes, c.var_nodes, c.codes, slot, c.starts, along) for along in (False, True))


def spelled(c, slot):
    return spec_haplotype_paths.spell(c.graph, c.ref_nodes, c.var_nodes, c.codes, slot, c.starts)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_segments_are_the_dirty_windows_each_once(name, k):
    c = case(name)
    for slot in range(c.n_slots):
        for bounds, intervals in both_walks(c, slot):
            starts = spec.window_starts(spec.segments(bounds, intervals, k))
            assert starts == sorted(set(starts)), (name, k, slot)
            assert starts == spec.dirty_windows(bounds, intervals, k), (name, k, slot)


def table_of(strings, k, n_nodes, seed):
    """bytes -> nodes from the windows of `strings`: a third of the distinct windows, one to three seeded nodes each."""
    rng = np.random.default_rng(seed)
    table = {}
    for s in strings:
        text = s.tobytes()
        for i in range(0, len(text) - k + 1):
            w = text[i:i + k]
            if w not in table and rng.random() < 0.34:
                table[w] = rng.integers(0, n_nodes + 3, size=int(rng.integers(1, 4))).tolist()     # some beyond n_nodes
    return table


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_base_minus_removed_plus_added_counts_every_window(name, k):
    c = case(name)
    n_nodes = 23
    base_strings = spelled(c, 0)
    table = table_of(base_strings + spelled(c, 1) + spelled(c, 2), k, n_nodes, [k, len(name)])
    base_letters = np.concatenate(base_strings)
    for rc in (True, False):
        base = None
        for slot in range(c.n_slots):
            strings = spelled(c, slot)
            letters = np.concatenate(strings)
            (ref_bounds, ref_iv), (bounds, iv) = both_walks(c, slot)
            assert bounds == np.concatenate([[0], np.cumsum([len(s) for s in strings])]).tolist()
            assert ref_bounds == np.concatenate([[0], np.cumsum([len(s) for s in base_strings])]).tolist()
            if base is None:
                assert not iv and not ref_iv                # slot 0 takes no line
                base = spec.count_windows(base_letters, spec.all_window_starts(ref_bounds, k), table, k, n_nodes, rc)
                assert base.sum() > 0
            want = spec.count_windows(letters, spec.all_window_starts(bounds, k), table, k, n_nodes, rc)
            removed = spec.count_windows(base_letters, spec.window_starts(spec.segments(ref_bounds, ref_iv, k)), table, k, n_nodes, rc)
            added = spec.count_windows(letters, spec.window_starts(spec.segments(bounds, iv, k)), table, k, n_nodes, rc)
            assert np.all(base - removed >= 0), (name, k, slot, rc)
            assert np.array_equal(base - removed + added, want), (name, k, slot, rc)


def formula_segments(plan, codes, slot, k):
    """What the kernels evaluate, from the plan's host arrays: the two segment lists."""
    kept = plan["kept_line"]
    alt = codes[kept, slot] == 1 if len(kept) else np.zeros(0, bool)
    ref_before = np.concatenate([[0], np.cumsum(plan["alt_size"], dtype=np.int64)])
    before = np.concatenate([[0], np.cumsum(np.where(alt, plan["ref_size"], plan["alt_size"]), dtype=np.int64)])
    cut = np.where(alt, plan["ref_start"], plan["alt_start"]) - before[:-1]
    ref_bounds = plan["chrom_seq_start"] - ref_before[plan["chrom_first_kept"]]
    bounds = plan["chrom_seq_start"] - before[plan["chrom_first_kept"]]
    out = ([], [])
    prev = [0, 0]
    for j in np.flatnonzero(alt).tolist():
        c = int(np.searchsorted(plan["chrom_first_kept"], j, side="right")) - 1
        a_ref = int(plan["ref_start"][j] - ref_before[j])
        for which, (a, size, bnd) in enumerate(((a_ref, int(plan["ref_size"][j]), ref_bounds),
                                                (int(cut[j]), int(plan["alt_size"][j]), bounds))):
            lo, hi = max(a - k + 1, prev[which], int(bnd[c])), min(a + size - 1, int(bnd[c + 1]) - k)
            if hi >= lo:
                out[which].append((lo, hi - lo + 1))
            prev[which] = a + size
    return out


@pytest.mark.parametrize("name", CASE_NAMES)
def test_the_plan_formula_gives_the_segments_of_the_walk(name):
    c = case(name)
    plan = hp.bubble_chain_plan(c.graph, VariantToNodesArrays(c.ref_nodes, c.var_nodes))
    for k in KS:
        for slot in range(c.n_slots):
            walked = tuple(spec.segments(b, iv, k) for b, iv in both_walks(c, slot))
            assert formula_segments(plan, c.codes, slot, k) == walked, (name, k, slot)


def test_census_of_the_cases():
    """The shapes the segment and probe kernels can go wrong at are among the cases, for both k."""
    for k in KS:
        windows, empty_ref, empty_alt, taken, short, clipped_lo, clipped_hi, merged = set(), 0, 0, set(), 0, 0, 0, 0
        for name in CASE_NAMES:
            c = case(name)
            for slot in range(c.n_slots):
                (ref_bounds, ref_iv), (bounds, iv) = both_walks(c, slot)
                taken.add(len(iv))
                empty_ref += sum(a == b for _, a, b in ref_iv)
                empty_alt += sum(a == b for _, a, b in iv)
                short += sum(b - a < k for a, b in zip(bounds[:-1], bounds[1:]))
                for bnd, ivs in ((ref_bounds, ref_iv), (bounds, iv)):
                    segs = spec.segments(bnd, ivs, k)
                    windows.update(n for _, n in segs)
                    clipped_lo += sum(a - k + 1 < bnd[ch] for ch, a, b in ivs)
                    clipped_hi += sum(b - 1 > bnd[ch + 1] - k for ch, a, b in ivs)
                    merged += sum(a2 - k + 1 < b1 for (_, _, b1), (_, a2, _) in zip(ivs[:-1], ivs[1:]))
        assert {1, 64, 65} <= windows and max(windows) > 128, (k, sorted(windows))
        assert {0, 63, 64, 65, 129, 300} <= taken and empty_ref > 0 and empty_alt > 0 and short > 0
        assert clipped_lo > 0 and clipped_hi > 0 and merged > 0


def test_the_model_on_a_hand_worked_example():
    # two kept lines (nodes 2 | 3 and 6 | 7) and one that is not kept; three diploid individuals
    ref_nodes, var_nodes = [2, 0, 6], [3, 0, 7]
    codes = np.array([[0, 0, 0, 1, 1, 1],
                      [1, 1, 1, 1, 1, 1],
                      [2, 1, 3, 0, 1, 1]], dtype=np.uint8)
    rows = [np.array([0, 0, 9, 0, 0, 0, 1, 2]), np.array([0, 0, 4, 3, 0, 0, 5, 0]), np.array([0, 0, 0, 2, 0, 0, 0, 700])]
    histogram, count_sum = spec.model(rows, codes, ref_nodes, var_nodes, [0, 1, 2], 2, 5)
    assert histogram.shape == (3, 2, 3, 5) and count_sum.shape == (3, 2, 3)
    assert histogram.dtype == np.uint32 and count_sum.dtype == np.uint64
    assert not histogram[1].any() and not count_sum[1].any()              # the line that is not kept
    # line 0: individual 0 is hom-ref (2 ref copies, 0 alt), 1 is het, 2 is hom-alt
    assert histogram[0][0].tolist() == [[1, 0, 0, 0, 0], [0, 0, 0, 0, 1], [0, 0, 0, 0, 1]]        # ref node 2: 0, 4, 9 (clipped)
    assert count_sum[0][0].tolist() == [0, 4, 9]
    assert histogram[0][1].tolist() == [[1, 0, 0, 0, 0], [0, 0, 0, 1, 0], [0, 0, 1, 0, 0]]        # var node 3: 0, 3, 2
    assert count_sum[0][1].tolist() == [0, 3, 2]
    # line 2: codes 2 and 3 follow the ref: individual 0 has one alt copy, 1 has none, 2 has two
    assert count_sum[2][0].tolist() == [0, 1, 5] and count_sum[2][1].tolist() == [0, 2, 700]
    assert histogram[2][1][2].tolist() == [0, 0, 0, 0, 1]                 # 700 goes to the last bin
    # two bins: everything above 0 is clipped into bin 1; a subset in another order
    histogram, count_sum = spec.model([rows[2], rows[0]], codes, ref_nodes, var_nodes, [2, 0], 2, 2)
    assert histogram[0][0].tolist() == [[1, 0], [0, 0], [0, 1]] and count_sum[0][0].tolist() == [0, 0, 9]
    # the same matrix as six haploid individuals: copies are 0 or 1
    histogram, count_sum = spec.model([rows[0]] * 6, codes, ref_nodes, var_nodes, range(6), 1, 5)
    assert histogram.shape == (3, 2, 2, 5) and histogram[0][0].sum(axis=1).tolist() == [3, 3]


def test_the_model_class_mean_and_files(tmp_path):
    histogram = np.zeros((2, 2, 3, 4), dtype=np.uint32)
    count_sum = np.zeros((2, 2, 3), dtype=np.uint64)
    histogram[0, 1, 2] = [1, 0, 2, 1]
    count_sum[0, 1, 2] = 30
    m = hp.NodeCountModel(histogram.reshape(-1), count_sum.reshape(-1), 31, 2, 4, [5, 0, 2, 3])
    assert m.histogram.shape == (2, 2, 3, 4) and m.count_sum.shape == (2, 2, 3)
    mean = m.mean()
    assert mean.shape == (2, 2, 3) and mean[0, 1, 2] == 7.5 and np.isnan(mean).sum() == 11
    m.to_file(str(tmp_path / "model"))
    back = hp.NodeCountModel.from_file(str(tmp_path / "model"))
    assert np.array_equal(back.histogram, m.histogram) and np.array_equal(back.count_sum, m.count_sum)
    assert back.histogram.dtype == np.uint32 and back.count_sum.dtype == np.uint64
    assert (back.k, back.ploidy, back.n_bins, back.samples.tolist()) == (31, 2, 4, [5, 0, 2, 3])
    assert sorted(np.load(str(tmp_path / "model.npz")).files) == ["count_sum", "histogram", "k", "n_bins", "ploidy", "samples"]
    empty = hp.NodeCountModel(np.zeros(0, np.uint32), np.zeros(0, np.uint64), 5, 1, 2, [])
    assert empty.histogram.shape == (0, 2, 2, 2) and empty.mean().shape == (0, 2, 2)


def test_whole_segments_cover_every_window_once():
    start, windows = hp.whole_segments(np.array([0, 40, 44, 100]), 5, windows=16)
    assert start.dtype == np.int64 and windows.dtype == np.int64 and windows.max() == 16
    assert spec.window_starts(zip(start.tolist(), windows.tolist())) == list(range(0, 36)) + list(range(44, 96))
    start, windows = hp.whole_segments(np.array([0, 4, 8]), 5)
    assert len(start) == 0 and len(windows) == 0


def test_the_host_argument_checks():
    """The checks come before the first device call, so a plan that is not there shows them."""
    paths = hp.HaplotypePaths.__new__(hp.HaplotypePaths)
    paths._plan, paths._alt_bits, paths._owns_plane, paths._ref_path, paths._base_rows = object(), None, False, None, {}
    paths.n_slots, paths.n_lines, paths.ploidy = 6, 3, 2
    try:
        for n_bins in (1, 0, -3):
            with pytest.raises(ValueError, match="n_bins"):
                paths.node_count_model(None, 31, n_bins=n_bins)
        for samples in ([3], [0, -1]):
            with pytest.raises(IndexError):
                paths.node_count_model(None, 31, samples=samples)
        with pytest.raises(ValueError, match="route"):
            paths.node_count_model(None, 31, route="both")
        with pytest.raises(ValueError, match="ploidy"):
            paths.node_count_model(None, 31, ploidy=1)
        with pytest.raises(IndexError):
            paths.node_counts_by_difference([0, 6], None, 31)
        paths.ploidy = None
        with pytest.raises(ValueError, match="ploidy="):
            paths.node_count_model(None, 31)
        with pytest.raises(IndexError):
            paths.node_count_model(None, 31, samples=[2], ploidy=3)
    finally:
        paths._plan = None
    with pytest.raises(ValueError, match="closed"):
        paths.reference_node_counts(None, 31, 10)


def test_the_parser_knows_the_new_sub_command_and_the_route():
    p = build_parser()
    a = p.parse_args(["make_node_count_model", "-g", "g", "-V", "v", "-m", "m", "-i", "i", "-o", "o"])
    assert (a.kmer_index, a.kmer_size, a.samples, a.n_bins, a.include_reverse_complement, a.route, a.out_file_name,
            a.func.__name__) == ("i", 31, None, 5, True, "difference", "o", "make_node_count_model")
    a = p.parse_args(["make_node_count_model", "-g", "g", "-V", "v", "-m", "m", "-i", "i", "-k", "5", "-s", "0,1,5", "-b", "2",
                      "-r", "False", "--route", "whole", "-o", "o"])
    assert (a.kmer_size, a.samples, a.n_bins, a.include_reverse_complement, a.route) == (5, "0,1,5", 2, False, "whole")
    a = p.parse_args(["haplotype_node_counts", "-g", "g", "-V", "v", "-m", "m", "-i", "i", "-s", "0"])
    assert a.route == "whole"
    a = p.parse_args(["haplotype_node_counts", "-g", "g", "-V", "v", "-m", "m", "-i", "i", "-s", "0", "--route", "difference"])
    assert a.route == "difference"
