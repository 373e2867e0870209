"""The boundary walk's step rule (csrc/gki_finder.hip: walk_entry, step_enters, step_windows, PathTopT, LevelStackT) is one body under the
count kernel and the emit kernel.  These hand-made graphs take both kernels through the branches of that rule which the
random-graph tests reach only by chance, in the classes that compile it differently -- the plain and the general kernels
(forced here on graphs that do not need them), with and without lossy restart points, one-node and all-nodes mode, the
product kernels and the slow path for deep windows -- against the plain-Python statements of the finder
(tests/spec_general.py, tests/spec_bruteforce.py).

CPU part: the graphs are what they are meant to be (flags of spec_general.classify, restart points, window depths), and the
two plain-Python statements agree where both apply.  GPU part (-m gpu): the finder's records."""
from collections import Counter

import numpy as np
import pytest

import spec_bruteforce
import spec_general
from spec_general import FORCED, T, SIMPLE, NESTED, HFS, DEAD
from graph_kmer_index_amd import GraphArrays
from oracle import oracle

# ---- empty nodes and the variant limit: two deletion sites in a row (nodes 2 and 4 are empty), then a SNP (6 / 7)
#   0 -> {1 | 2 ""} -> {3 | 4 ""} -> 5 -> {6 | 7} -> 8
# end node 5: an empty predecessor at level 1 (4) and one below an empty node (2); windows over 4 and 2 hold two variant
# nodes, those of end node 7 (itself a variant node: the first non-free node is level 0) three -- with M = 1, 2, 3 every
# one of them is once at M and once at M + 1.  End nodes 5, 6 and 8 meet their first non-free node at level 1 or deeper.
INDELS = dict(seqs={0: "ACGTACGT", 1: "G", 2: "", 3: "T", 4: "", 5: "AC", 6: "A", 7: "C", 8: "GGTCA"},
              edges={0: [1, 2], 1: [3, 4], 2: [3, 4], 3: [5], 4: [5], 5: [6, 7], 6: [8], 7: [8]}, linear=[0, 1, 3, 5, 6, 8])

# ---- only_follow_nodes = {4}: node 2 has a forced successor (HFS), so its edges to 3 and 5 do not exist for the search
#   0 -> {1 | 2};  1 -> 3;  2 -> {3, 4, 5};  {3, 4, 5} -> 6 -> 7 -> 8 -> 9
# 5 is DEAD (its only predecessor is 2, and 5 is not forced); 3 lives through 1.  The HFS predecessor 2 is met under the
# unforced parent 3 and under the forced parent 4, with that parent at level 0 (end nodes 3, 4), 1 (end node 6), 2 (7),
# 3 (8) and 4 (9): the four arms of PathTopT::node_at and the array behind them.
FORCED_SITE = dict(seqs={0: "ACGTACG", 1: "G", 2: "C", 3: "A", 4: "T", 5: "G", 6: "G", 7: "T", 8: "A", 9: "CCGTA"},
                   edges={0: [1, 2], 1: [3], 2: [3, 4, 5], 3: [6], 4: [6], 5: [6], 6: [7], 7: [8], 8: [9]},
                   linear=[0, 1, 3, 6, 7, 8, 9], follow={4})

# ---- a bubble inside an alternative allele: 3 and 4 have no T predecessor (NESTED)
#   0 -> {1 | 2};  2 -> {3 | 4} -> 5 -> 6;  {1, 6} -> 7
# k = 5: the windows of end node 7 at offsets 0 and 1 begin inside 3 / 4, which are level 3 of the walk (7, 6, 5, 3).  With
# M = 100 the history bound in the flag word decides (fq >> 8); with M = 4 it does not and history_ok is called with the
# path's levels 1 and 2 still in registers: the flush.  M = 3: node 5 is at the limit with no linear-ref successor (:402).
NESTED_SITE = dict(seqs={0: "ACGTACGT", 1: "ACG", 2: "T", 3: "CA", 4: "GG", 5: "A", 6: "G", 7: "TTGCA"},
                   edges={0: [1, 2], 1: [7], 2: [3, 4], 3: [5], 4: [5], 5: [6], 6: [7]}, linear=[0, 1, 7])

# ---- restart points inside nodes: the reference segment after each SNP is cut into short nodes, so that the critical
# point k - 1 bases behind the bubble lies inside one (0 < c < k - 1), and the next node's windows would reach before it
CUT_SEGMENTS = dict(seqs={0: "ACGTACG", 1: "A", 2: "C", 3: "GT", 4: "ACGT", 5: "CA", 6: "G", 7: "T", 8: "T", 9: "GCATA", 10: "ACCGTGA"},
                    edges={0: [1, 2], 1: [3], 2: [3], 3: [4], 4: [5], 5: [6, 7], 6: [8], 7: [8], 8: [9], 9: [10]},
                    linear=[0, 1, 3, 4, 5, 6, 8, 9, 10])


def empty_run(n_empty):
    """n_empty linear-ref dummy nodes between two segments: the windows of the last node cross n_empty + 2 nodes."""
    seqs = {0: "ACGTACGT"}
    seqs.update({i: "" for i in range(1, n_empty + 1)})
    seqs[n_empty + 1] = "CCGTA"
    return dict(seqs=seqs, edges={i: [i + 1] for i in range(n_empty + 1)}, linear=list(range(n_empty + 2)))


def graph_of(case):
    return GraphArrays.from_dicts(case["seqs"], case["edges"], case["linear"], case.get("af"))


def rows_of(cols):
    return Counter(zip(np.asarray(cols["kmers"]).tolist(), np.asarray(cols["start_nodes"]).tolist(), np.asarray(cols["start_offsets"]).tolist(),
                       np.asarray(cols["nodes"]).tolist(), np.asarray(cols["allele_frequencies"]).tolist()))


_SPEC = {}


def expected(case, k, M, one, critical=None, store=None):
    """Counter of the records per spec_general, or 'assert'.  only_store_nodes (kmer_finder.py:145-154) keeps, of a
    window's records, those of nodes in the set; no node of these graphs is long enough for the bulk path that ignores it."""
    key = (repr(case), k, M, one, None if critical is None else tuple(sorted(critical.items())))
    if key not in _SPEC:            # computed once, shared by the CPU and the GPU tests, never changed
        try:
            _SPEC[key] = spec_general.spec_rows_general(graph_of(case), k, M, one, critical=critical, follow=case.get("follow"))
        except spec_general.SpecError:
            _SPEC[key] = "assert"
    rows = _SPEC[key]
    if store is None or rows == "assert":
        return rows
    assert max(len(s) for s in case["seqs"].values()) <= 2 * k + 3
    return Counter({r: c for r, c in rows.items() if r[3] in store})


def critical_of(case, k):
    cn, co = oracle.critical_paths(graph_of(case), k)
    return (cn, co), {int(n): int(c) for n, c in zip(cn, co)}


# (case, k, M values, chunked at the critical points?, only_store_nodes)
RUNS = [("indels", INDELS, 5, (1, 2, 3), False, None),
        ("forced_site", FORCED_SITE, 7, (2,), False, None),
        ("forced_site_store", FORCED_SITE, 7, (2,), False, {0, 2, 4, 7}),
        ("nested_site", NESTED_SITE, 5, (3, 4, 100), False, None),
        ("nested_site_store", NESTED_SITE, 5, (4,), False, {3, 5, 7}),
        ("cut_segments", CUT_SEGMENTS, 5, (1,), True, None),
        ("empty_run_45", empty_run(45), 5, (1,), False, None),        # the first segment is level 46 = MAXN - 2: the last that fits
        ("empty_run_46", empty_run(46), 5, (1,), False, None)]        # level 47: GKI_ERR_WINDOW_TOO_DEEP, the slow path answers


def test_the_graphs_are_what_they_are_meant_to_be():
    flags = lambda case, k, M: spec_general.classify(graph_of(case), k, M, case.get("follow"))
    f = flags(FORCED_SITE, 7, 2)
    assert f[2] & HFS and f[5] & DEAD and f[4] & FORCED and not f[3] & (FORCED | DEAD) and not f[1] & HFS
    f = flags(NESTED_SITE, 5, 4)
    assert f[3] & NESTED and f[4] & NESTED and f[2] & SIMPLE and f[0] & T and not any(x & DEAD for x in f)
    assert expected(NESTED_SITE, 5, 3, True) == "assert" and expected(NESTED_SITE, 5, 4, True) != "assert"
    # the walk of end node 7 begins a window inside 3, three levels up
    assert any(r[1] == 7 and r[3] == 3 for r in expected(NESTED_SITE, 5, 4, False))
    # the limit cuts: every M of the case changes the records of end node 5 (two variant nodes) or 7 (three)
    per_M = [expected(INDELS, 5, M, False) for M in (1, 2, 3)]
    assert sum(per_M[0].values()) < sum(per_M[1].values()) < sum(per_M[2].values())
    windows_over = lambda rows, nodes: set.intersection(*[{r[:3] for r in rows if r[3] == x} for x in nodes])
    assert not windows_over(per_M[0], (2, 4)) and any(w[1] == 5 for w in windows_over(per_M[1], (2, 4)))
    assert not windows_over(per_M[1], (2, 4, 7)) and windows_over(per_M[2], (2, 4, 7))
    # restart points inside nodes, and a node right behind one that is shorter than k - 1
    _, critd = critical_of(CUT_SEGMENTS, 5)
    inside = {n: c for n, c in critd.items() if 0 < c < 4}
    assert len(inside) >= 2, critd
    g = graph_of(CUT_SEGMENTS)
    assert any(int(g.node_size[n]) - c < 4 for n, c in inside.items()), (critd, g.node_size)
    # the two plain-Python statements agree where both apply (no only_follow_nodes, every node with a linear-ref predecessor)
    for case, k, M in ((INDELS, 5, 2), (CUT_SEGMENTS, 5, 1), (empty_run(45), 5, 1)):
        crit = critical_of(case, k)[1] if case is CUT_SEGMENTS else None
        for one in (True, False):
            assert expected(case, k, M, one, crit) == spec_bruteforce.spec_rows(graph_of(case), k, M, one, critical=crit)
    assert len(empty_run(46)["seqs"]) == 48 and any(r[1] == 47 and r[3] == 0 for r in expected(empty_run(46), 5, 1, False))


@pytest.mark.gpu
@pytest.mark.parametrize("general", [False, True], ids=["plain", "general"])
@pytest.mark.parametrize("one", [True, False], ids=["one_node", "all_nodes"])
@pytest.mark.parametrize("name,case,k,Ms,chunked,store", RUNS, ids=[r[0] for r in RUNS])
def test_both_kernels_follow_the_rule(name, case, k, Ms, chunked, store, one, general):
    from graph_kmer_index_amd import CriticalGraphPaths, DenseKmerFinder
    from gpu_util import finder_cols
    g = graph_of(case)
    crit, critd = critical_of(case, k) if chunked else (None, None)
    n_chunks = len(crit[0]) if chunked else 1          # contiguous ranges of critical-path numbers (command_line_interface.py:588-601)

    def run(M, chunk):
        kw = dict(only_save_one_node_per_kmer=one, max_variant_nodes=M, only_follow_nodes=case.get("follow"), only_store_nodes=store)
        if chunked:
            kw.update(critical_graph_paths=CriticalGraphPaths(*crit), start_at_critical_path_number=chunk,
                      stop_at_critical_path_number=chunk + 1)
        f = DenseKmerFinder(g, k, **kw)
        f._force_general_kernels = general
        f.find()
        return rows_of(finder_cols(f))

    for M in Ms:
        want = expected(case, k, M, one, critd, store)
        if want == "assert":
            with pytest.raises(AssertionError):
                run(M, 0)
            continue
        got = Counter()
        for chunk in range(n_chunks):          # runs that begin and end inside nodes; together they are the whole graph
            got += run(M, chunk)
        assert got == want, (name, M, sorted((got - want).items())[:5], sorted((want - got).items())[:5])
