"""The device critical-path walk (csrc/gki_critical.hip, gki_graph_critical_paths) on both of its routes, past one
block of its scans and past one round of its grid-stride loops, against the plain Python spec (tests/spec_critical.py):
values, order, dtypes; on errors the kind and the node named in the message.

Which route ran cannot be observed from outside the library; tests/critical_cases.py forces it by construction (see its
docstring).  Every case runs on THE GUESS as built and on THE FALLBACK (jump tables + k_walk_fill) under the
relabellings "random", "reversed", "swap_last" and, where the path has three nodes, "swap_first".  The two large cases
(f, g) compare with the library's host walk, which tests/test_critical_spec.py pins to the spec on everything smaller.

  (a) scan block edges: paths of 2047, 2048, 2049 and 4097 nodes                       guess + 4 relabellings
  (b) k_walk_fill levels and `top`: chromosomes of 1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33 and 1025 path nodes in one call, and
      the list reversed                                                                guess + 4 relabellings
  (c) chromosome starts out of id order: [C, A, B]                                     guess
      a second component that is not listed                                            fallback (the guess is rejected)
      only the second component relabelled                                             fallback
  (d) 64 chromosomes                                                                   guess + 4 relabellings
      65: refused on the device, the host walk without asking for the device
  (e) the walk's state on 300 random graphs                                            guess + a random permutation each
  (f) more than 524 288 nodes and path nodes: a second round of every grid-stride loop  guess + 3 relabellings
      the two errors behind it in either order                                         guess + random permutation
  (g) a path of more than 2048 * 2048 + 2048 nodes: three scan levels                  guess + 3 relabellings
  (h) a cycle                                                                          fallback
"""
import time

import numpy as np
import pytest

import critical_cases as cc
import spec_critical as spec
from graph_kmer_index_amd import CriticalGraphPaths

pytestmark = pytest.mark.gpu


def device(g, k):
    return cc.library_outcome(g, k, on_device=True)


def host(g, k):
    return cc.library_outcome(g, k, on_device=False)


@pytest.mark.parametrize("path_len", cc.SCAN_EDGE_LENGTHS)
def test_a_scan_block_edges(path_len):
    g = cc.scan_edge_graph(path_len)
    path = cc.longest_path(g, cc.K_SMALL)
    assert len(path) == path_len
    cc.check_against_spec(g, cc.K_SMALL, device, cc.relabellings(g.n_nodes, path))


@pytest.mark.parametrize("reverse", [False, True])
def test_b_fill_levels_with_chromosomes_of_unequal_length(reverse):
    parts = list(cc.fill_components())[::-1 if reverse else 1]
    g = cc.concat(parts)
    paths = spec.walk(g, cc.K_SMALL)[0]
    assert [len(p) for p in paths] == list(cc.FILL_LENGTHS)[::-1 if reverse else 1]
    want = cc.check_against_spec(g, cc.K_SMALL, device, cc.relabellings(g.n_nodes, max(paths, key=len)))
    bounds = np.cumsum([0] + [p.n_nodes for p in parts])
    assert np.all(np.diff(np.searchsorted(bounds, want[0], side="right")) >= 0)      # in the order of the list


def test_c_chromosome_starts_out_of_id_order():
    a, b, c = cc.three_components()
    whole = cc.concat([a, b, c])
    sa, sb, sc = whole.chromosome_start_nodes.values()
    want = cc.check_against_spec(cc.with_starts(whole, [sc, sa, sb]), cc.K_SMALL, device)
    assert want[0][0] >= sc and want[0][-1] < sc
    # b is not listed: its linear-ref nodes sit in a's guessed slice, the guess must be rejected
    assert cc.check_against_spec(cc.with_starts(cc.concat([a, b]), [0]), cc.K_SMALL, device) == spec.outcome(a, cc.K_SMALL)
    for name, p in cc.relabellings(b.n_nodes, cc.longest_path(b, cc.K_SMALL)).items():
        cc.check_against_spec(cc.block_relabel((a, b), 1, lambda n, p=p: p), cc.K_SMALL, device)


def test_d_64_chromosomes_and_one_more():
    g = cc.many_chromosomes(64)
    assert len(g.chromosome_start_nodes) == 64
    cc.check_against_spec(g, cc.K_SMALL, device, cc.relabellings(g.n_nodes, cc.longest_path(g, cc.K_SMALL)))
    g = cc.many_chromosomes(65)
    assert len(g.chromosome_start_nodes) == 65
    with pytest.raises(Exception, match="1..64"):
        CriticalGraphPaths.from_graph(g, cc.K_SMALL, on_device=True)
    assert cc.library_outcome(g, cc.K_SMALL, on_device=None) == spec.outcome(g, cc.K_SMALL)


def test_e_walk_state_on_random_graphs():
    n_ok = n_raise = 0
    for it, k, g, perm, moved in cc.state_graphs():
        want = cc.check_against_spec(g, k, device, {"random": perm}, want_values=False)
        n_raise += want[0] == "raises"
        n_ok += want[0] != "raises"
    assert n_ok >= 200 and n_raise >= 5          # (tests/test_critical_spec.py asserts the same census on the CPU)


# ------------------------------------------------------------------------------------------------ the large cases
LARGE_ROUTES = ("guess", "random", "reversed", "swap_last")


def check_large(g, route):
    """the device equals the host walk on the graph itself; a relabelled graph's result is the as-built one renamed"""
    t0 = time.perf_counter()
    want = host(g, cc.K_LARGE)
    assert want[0] != "raises" and len(want[0]) > 100_000
    if route != "guess":
        perm = cc.relabellings(g.n_nodes, cc.ref_path(g))[route]
        g = cc.relabel(g, perm)
        want_moved = host(g, cc.K_LARGE)
        assert want_moved == cc.renamed(want, perm)
        want = want_moved
    t1 = time.perf_counter()
    got = device(g, cc.K_LARGE)
    t2 = time.perf_counter()
    print("%s: %d nodes, %d critical points; host side %.2f s, device call (with the upload) %.2f s"
          % (route, g.n_nodes, len(want[0]), t1 - t0, t2 - t1))
    assert got == want


@pytest.mark.parametrize("route", LARGE_ROUTES)
def test_f_second_round_of_the_grid_stride_loops(route):
    g = cc.second_round_graph()
    assert g.n_nodes > cc.GRID_THREADS and len(cc.ref_path(g)) > cc.GRID_THREADS
    check_large(g, route)


@pytest.mark.parametrize("route", ("guess", "random"))
@pytest.mark.parametrize("name", ("offset_then_branch", "branch_then_offset", "offset_alone"))
def test_f_a_branch_error_beats_an_offset_error_at_scale(name, route):
    g, kind, node = cc.error_precedence_cases(cc.second_round_graph())[name]
    want = ("raises", kind, node)
    if route != "guess":
        perm = cc.relabellings(g.n_nodes, cc.ref_path(cc.second_round_graph()))[route]
        g, want = cc.relabel(g, perm), cc.renamed(want, perm)
    assert host(g, cc.K_LARGE) == want
    assert device(g, cc.K_LARGE) == want


@pytest.mark.parametrize("route", LARGE_ROUTES)
def test_g_three_scan_levels(route):
    g = cc.three_level_graph()
    assert len(cc.ref_path(g)) > cc.SCAN_TILE * cc.SCAN_TILE + cc.SCAN_TILE
    check_large(g, route)


def test_h_a_cycle_is_refused():
    g = cc.cycle_graph()
    with pytest.raises(Exception, match="left the graph or found a cycle"):
        CriticalGraphPaths.from_graph(g, 3, on_device=True)
    with pytest.raises(Exception, match="left the graph or found a cycle"):
        CriticalGraphPaths.from_graph(g, 3, on_device=False)
    assert spec.outcome(g, 3)[:2] == ("raises", "cycle")
