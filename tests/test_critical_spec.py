"""tests/spec_critical.py -- the plain Python restatement of CriticalGraphPaths.from_graph -- pinned to the reference's
known answers, the reference-generated fixtures, the recorded order of its two errors and the oracle; the graph helpers
of tests/critical_cases.py; and the library's host walk (gki_critical_paths) pinned to the spec on every small case of
the GPU route tests (tests/test_gpu_critical_paths_routes.py compares the device with the same expectations)."""
import json
import os

import numpy as np
import pytest

import critical_cases as cc
import spec_critical as spec
from golden_cases import CRITICAL_KATS
from graph_kmer_index_amd.graph import GraphArrays
from graphgen import random_bubble_graph, nested_bubble_graph, deep_nested_graph, overlapping_bubble_graph
from oracle import oracle

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def host(g, k):
    return cc.library_outcome(g, k, on_device=False)


# ------------------------------------------------------------------------------------------------ the spec itself
@pytest.mark.parametrize("name", sorted(CRITICAL_KATS))
def test_spec_gives_the_reference_known_answers(name):
    (seqs, edges, lin), k, nodes, offsets = CRITICAL_KATS[name]
    got_nodes, got_offsets = spec.critical_paths(GraphArrays.from_dicts(seqs, edges, lin), k)
    assert got_nodes.tolist() == nodes and got_offsets.tolist() == offsets
    assert got_nodes.dtype == np.uint32 and got_offsets.dtype == np.uint16


@pytest.mark.parametrize("fixture", ["finder_toy.json", "finder_two_chrom.json"])
def test_spec_gives_the_reference_generated_fixtures(fixture):
    with open(os.path.join(GOLD, fixture)) as f:
        cases = json.load(f)
    seen = raised = 0
    for case in cases:
        if ("crit_nodes" not in case and case.get("raises") != "E2") or "from_position" in case.get("kw", {}):
            continue                 # (early-stop cases carry no critical points: the reference runs them without)
        g = GraphArrays.from_dicts({int(a): b for a, b in case["seqs"].items()}, {int(a): b for a, b in case["edges"].items()},
                                   case["linear"], chromosome_start_nodes=case.get("chromosome_start_nodes"))
        got = spec.outcome(g, case["k"])
        if case.get("raises") == "E2":
            assert got[:2] == ("raises", "offset"), case["name"]
            raised += 1
        else:
            assert got == (case["crit_nodes"], case["crit_offsets"]), case["name"]
            seen += 1
    assert seen > 50 and (raised > 0 or fixture == "finder_toy.json")


def _error_order_cases():
    with open(os.path.join(GOLD, "critical_error_order.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("case", _error_order_cases(), ids=lambda c: c["name"])
def test_a_branch_error_beats_an_offset_error_as_recorded_from_the_reference(case):
    """tests/golden/make_golden_critical_errors.py: with both errors in a graph the reference raises the branch error
    (inside the walk), wherever the offset of -1 sits; the spec, the host walk and the oracle follow it."""
    g = GraphArrays.from_dicts({int(a): b for a, b in case["seqs"].items()}, {int(a): b for a, b in case["edges"].items()},
                               case["linear"], chromosome_start_nodes=case["chromosome_start_nodes"])
    got = spec.outcome(g, case["k"])
    assert got[:2] == ("raises", case["kind"])
    if case["node"] is not None:
        assert got[2] == case["node"]
    assert host(g, case["k"]) == got
    with pytest.raises(oracle.OracleError) as e:
        oracle.critical_paths(g, case["k"])
    assert e.value.code == {"branch": 3, "offset": 4}[case["kind"]]


def test_both_orders_are_recorded():
    cases = {c["name"]: c for c in _error_order_cases()}
    assert cases["two_walks_offset_then_branch"]["raises"] == cases["two_walks_branch_then_offset"]["raises"] == "Exception"
    assert cases["one_walk_offset_then_branch"]["raises"] == "Exception" and cases["two_walks_offset_alone"]["raises"] == "OverflowError"


def test_spec_equals_the_oracle_on_random_graphs():
    """the 400 graphs of test_gpu_critical.test_random_graphs_equal_the_host_walk_and_the_oracle (none is cyclic)"""
    rng = np.random.default_rng(12)
    n_ok = n_raise = 0
    for it in range(400):
        kind = it % 4
        k = int(rng.integers(2, 12))
        if kind == 0:
            seqs, edges, lin, af = random_bubble_graph(rng, n_var=int(rng.integers(1, 9)), min_ref=1, max_ref=int(rng.integers(2, 3 * k)),
                                                       p_indel=0.4, chain_after={int(rng.integers(-1, 3)): int(rng.integers(1, k + 2))})
        elif kind == 1:
            seqs, edges, lin, af = nested_bubble_graph(rng, n_var=int(rng.integers(2, 7)), min_ref=1, max_ref=12, p_nest=0.6, p_chain=0.4)
        elif kind == 2:
            seqs, edges, lin, af = deep_nested_graph(rng, n_var=int(rng.integers(1, 5)), max_depth=2)
        else:
            seqs, edges, lin = overlapping_bubble_graph(rng)[:3]
        g = GraphArrays.from_dicts(seqs, edges, lin)
        got = spec.outcome(g, k)
        try:
            cn, co = oracle.critical_paths(g, k)
            assert got == (cn.tolist(), co.tolist()), it
            n_ok += 1
        except oracle.OracleError as e:
            assert got[:2] == ("raises", {3: "branch", 4: "offset"}[e.code]), it
            n_raise += 1
        assert host(g, k) == got, it
    assert n_ok > 250 and n_raise > 3


def test_spec_stops_on_a_cycle_and_so_does_the_host_walk():
    g = cc.cycle_graph()
    with pytest.raises(spec.SpecError) as e:
        spec.critical_paths(g, 3)
    assert e.value.kind == "cycle"
    assert host(g, 3)[:2] == ("raises", "cycle")


# ------------------------------------------------------------------------------------------------ relabel and concat
def _arrays(g):
    return [getattr(g, name) for name in ("node_size", "seq_start", "seq", "edge_start", "edges", "rev_start", "rev_edges",
                                          "is_ref", "allele_freq", "exists")] + \
        [np.array(list(g.chromosome_start_nodes.values())), np.array(g.first_node)]


def test_relabel_renames_every_array_and_comes_back():
    rng = np.random.default_rng(3)
    for it in range(40):
        seqs, edges, lin, af = random_bubble_graph(rng, n_var=int(rng.integers(1, 7)), with_af=True)
        g = GraphArrays.from_dicts(seqs, edges, lin, af)
        p = rng.permutation(g.n_nodes)
        moved = cc.relabel(g, p)
        direct = GraphArrays.from_dicts({int(p[a]): s for a, s in seqs.items()}, {int(p[a]): [int(p[x]) for x in e] for a, e in edges.items()},
                                        [int(p[a]) for a in lin], {int(p[a]): f for a, f in af.items()})
        for a, b in zip(_arrays(moved)[:-1], _arrays(direct)[:-1]):
            assert np.array_equal(a, b)
        for a, b in zip(_arrays(cc.relabel(moved, np.argsort(p))), _arrays(g)):
            assert np.array_equal(a, b)


def test_concat_lists_the_components_in_the_order_passed():
    rng = np.random.default_rng(4)
    lits = [random_bubble_graph(rng, n_var=n) for n in (2, 0, 3)]
    parts = [GraphArrays.from_dicts(*lit[:3]) for lit in lits]
    whole = cc.concat(parts)
    seqs, edges, lin, starts, shift = {}, {}, [], [], 0
    for (s, e, li, _), part in zip(lits, parts):
        seqs.update({a + shift: b for a, b in s.items()})
        edges.update({a + shift: [x + shift for x in b] for a, b in e.items()})
        lin += [a + shift for a in li]
        starts.append(shift)
        shift += part.n_nodes
    direct = GraphArrays.from_dicts(seqs, edges, lin, chromosome_start_nodes=starts)
    for a, b in zip(_arrays(whole), _arrays(direct)):
        assert np.array_equal(a, b)
    back = cc.concat(parts[::-1])
    assert list(back.chromosome_start_nodes.values()) == [0, parts[2].n_nodes, parts[2].n_nodes + parts[1].n_nodes]
    n0, o0 = spec.critical_paths(whole, 4)
    listed = cc.with_starts(whole, list(whole.chromosome_start_nodes.values())[::-1])
    n1, o1 = spec.critical_paths(listed, 4)
    assert sorted(zip(n0.tolist(), o0.tolist())) == sorted(zip(n1.tolist(), o1.tolist())) and len(n0) > 2


# ------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("path_len", cc.SCAN_EDGE_LENGTHS)
def test_case_a_scan_block_edges(path_len):
    g = cc.scan_edge_graph(path_len)
    path = cc.longest_path(g, cc.K_SMALL)
    assert len(path) == path_len and path == cc.ref_path(g).tolist()
    cc.check_against_spec(g, cc.K_SMALL, host, cc.relabellings(g.n_nodes, path))


@pytest.mark.parametrize("reverse", [False, True])
def test_case_b_fill_levels(reverse):
    parts = list(cc.fill_components())[::-1 if reverse else 1]
    g = cc.concat(parts)
    paths = spec.walk(g, cc.K_SMALL)[0]
    assert [len(p) for p in paths] == list(cc.FILL_LENGTHS)[::-1 if reverse else 1]
    want = cc.check_against_spec(g, cc.K_SMALL, host, cc.relabellings(g.n_nodes, max(paths, key=len)))
    # results come in the order of the chromosome list: chromosome by chromosome
    bounds = np.cumsum([0] + [p.n_nodes for p in parts])
    owner = np.searchsorted(bounds, want[0], side="right")
    assert np.all(np.diff(owner) >= 0) and len(set(owner.tolist())) > 6


def test_case_c_chromosome_starts_out_of_id_order():
    a, b, c = cc.three_components()
    whole = cc.concat([a, b, c])
    sa, sb, sc = whole.chromosome_start_nodes.values()
    listed = cc.with_starts(whole, [sc, sa, sb])
    want = cc.check_against_spec(listed, cc.K_SMALL, host)
    assert want[0][0] >= sc and want[0][-1] < sc
    first_only = cc.with_starts(cc.concat([a, b]), [0])
    assert cc.check_against_spec(first_only, cc.K_SMALL, host) == spec.outcome(a, cc.K_SMALL)
    path_b = cc.longest_path(b, cc.K_SMALL)
    for name, p in cc.relabellings(b.n_nodes, path_b).items():
        cc.check_against_spec(cc.block_relabel((a, b), 1, lambda n, p=p: p), cc.K_SMALL, host)


def test_case_d_chromosome_limits():
    for count in (64, 65):
        g = cc.many_chromosomes(count)
        assert len(g.chromosome_start_nodes) == count
        cc.check_against_spec(g, cc.K_SMALL, host)


def test_case_e_state_graph_census():
    """the seed of critical_cases.state_graphs gives, by the spec alone, at least 200 graphs that do not raise and at
    least 5 that do -- and the host walk equals the spec on every one, as built and permuted"""
    n_ok = n_raise = 0
    kinds = set()
    for it, k, g, perm, moved in cc.state_graphs():
        want = cc.check_against_spec(g, k, host, {"random": perm}, want_values=False)
        if want[0] == "raises":
            n_raise += 1
            kinds.add(want[1])
        else:
            n_ok += 1
    assert n_ok >= 200 and n_raise >= 5 and n_ok + n_raise == cc.STATE_GRAPHS
    assert "offset" in kinds
