"""The NumPy restatement of sample_kmers_from_structural_variants (tests/spec_structural_variants.py) against the
reference's own output (tests/golden/sv_kmers_reference.json.gz), and the features the fixture was planted with, asserted
on the stored data.  CPU only."""
import numpy as np
import pytest

import spec_structural_variants as spec

CASES = spec.load_cases()
BY_NAME = {c["name"]: c for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_spec_equals_reference(case):
    g = spec.case_graph(case)
    got = spec.sample_kmers(g, case["pairs"], spec.case_table(case), case["k"], case["max_frequency"])
    exp = spec.expected(case)
    for a, b in zip(got, exp[:3]):
        assert a.dtype == b.dtype
        assert np.array_equal(a, b)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_reference_dtypes_and_constant_columns(case):
    h, n, r, af = spec.expected(case)
    assert (h.dtype, n.dtype, r.dtype, af.dtype) == (np.uint64, np.uint32, np.uint32, np.float32)
    assert len(h) == len(n) == len(r) == len(af)
    assert not r.any() and np.all(af == 1.0)


def _sizes(case):
    return {int(n): len(s) for n, s in case["graph"]["node_sequences"].items()}


def _nodes(case):
    return [n for p in case["pairs"] for n in p]


def test_sizes_k_plus_5_skipped_and_k_plus_6_taken():
    case = BY_NAME["sizes_and_all_frequent"]
    k, sizes, out_nodes = case["k"], _sizes(case), set(case["expected"]["nodes"])
    at5 = [n for n in _nodes(case) if sizes[n] == k + 5]
    at6 = [n for n in _nodes(case) if sizes[n] == k + 6]
    assert at5 and at6
    assert not out_nodes & set(at5)
    assert set(at6) <= out_nodes


def test_a_node_whose_every_window_is_frequent_gives_no_record():
    case = BY_NAME["sizes_and_all_frequent"]
    g, table = spec.case_graph(case), spec.case_table(case)
    big = [n for n in _nodes(case) if _sizes(case)[n] > case["k"] + 5]
    none_valid = [n for n in big if len(spec.valid_windows(g, n, table, case["k"], case["max_frequency"])[1]) == 0]
    assert none_valid
    assert not set(none_valid) & set(case["expected"]["nodes"])


def test_frequencies_contributed_only_by_the_reverse_complement():
    hit = 0
    for case in CASES:
        g, table = spec.case_graph(case), spec.case_table(case)
        for n in set(_nodes(case)):
            if _sizes(case)[n] > case["k"] + 5:
                h = spec.window_hashes(g.get_numeric_node_sequence(n), case["k"])
                own, rc = table.first_hit(h), table.first_hit(spec.revcomp(h, 31))
                hit += int(((own == 0) & (rc >= case["max_frequency"])).sum())      # invalid by the reverse complement alone
    assert hit > 0


def test_k15_reverse_complement_at_31_changes_the_result():
    case = BY_NAME["k15_revcomp_quirk"]
    assert case["k"] == 15
    g, table = spec.case_graph(case), spec.case_table(case)
    quirk = spec.sample_kmers(g, case["pairs"], table, 15, case["max_frequency"], rc_k=31)
    true_rc = spec.sample_kmers(g, case["pairs"], table, 15, case["max_frequency"], rc_k=15)
    assert np.array_equal(quirk[0], spec.expected(case)[0])
    assert not np.array_equal(quirk[0], true_rc[0])


def test_max_frequencies_1_2_and_5():
    outs = {}
    for mf in (1, 2, 5):
        case = BY_NAME["max_frequency_%d" % mf]
        assert case["max_frequency"] == mf
        outs[mf] = case["expected"]["hashes"]
    assert BY_NAME["max_frequency_1"]["graph"] == BY_NAME["max_frequency_5"]["graph"]
    assert outs[1] != outs[2] and outs[2] != outs[5] and len(outs[1]) > 0


def test_valid_runs_force_the_greedy_rule():
    """Somewhere a window j is chosen, j + k - 1 and j + k are both valid, and j + k is the next one chosen."""
    hit = 0
    for case in CASES:
        g, table, k = spec.case_graph(case), spec.case_table(case), case["k"]
        for n in set(_nodes(case)):
            if _sizes(case)[n] > k + 5:
                valid = spec.valid_windows(g, n, table, k, case["max_frequency"])[1]
                chosen = spec.greedy(valid, k).tolist()
                vs = set(valid.tolist())
                hit += sum(1 for a, b in zip(chosen, chosen[1:]) if b == a + k and a + k - 1 in vs)
    assert hit > 0
    case = BY_NAME["greedy_rule"]
    valid = spec.valid_windows(spec.case_graph(case), 3, spec.case_table(case), 31, 2)[1]
    assert valid.tolist() == [10, 40, 41, 72, 102, 103]
    assert spec.greedy(valid, 31).tolist() == [10, 41, 72, 103]


def test_shared_nodes_ref_equals_var_and_node_0():
    case = BY_NAME["shared_nodes_and_no_node"]
    pairs, sizes, k = case["pairs"], _sizes(case), case["k"]
    nodes = _nodes(case)
    assert sizes[0] == 0
    assert any(r == 0 and v != 0 for r, v in pairs) and any(v == 0 and r != 0 for r, v in pairs) and [0, 0] in pairs
    same = [r for r, v in pairs if r == v and sizes[r] > k + 5]
    assert same
    twice = [n for n in set(nodes) if nodes.count(n) >= 2 and sizes[n] > k + 5 and
             any(n in p for p in pairs if p[0] != p[1])]
    assert twice
    out = case["expected"]["nodes"]
    for n in set(same + twice):                  # their records appear once per listing
        assert out.count(n) > 0 and out.count(n) % nodes.count(n) == 0
    assert 0 not in out


def test_a_node_longer_than_64_times_64_windows():
    for name in ("long_nodes_sparse", "long_nodes_dense"):
        case = BY_NAME[name]
        sizes, k = _sizes(case), case["k"]
        long_nodes = [n for n in _nodes(case) if sizes[n] - k + 1 > 64 * 64]
        assert long_nodes
        assert any(sizes[n] - k + 1 > 2 * 64 * 64 for n in long_nodes)
        out = np.array(case["expected"]["nodes"])
        assert all((out == n).sum() > 64 * 64 // (4 * k) for n in long_nodes)


def test_empty_input():
    case = BY_NAME["no_pairs"]
    assert case["pairs"] == [] and case["expected"]["hashes"] == []
    case = BY_NAME["only_small_nodes"]
    assert case["pairs"] and case["expected"]["hashes"] == []
