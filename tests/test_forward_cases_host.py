"""Census of tests/forward_cases.py from the oracle alone (no GPU): every boundary of the early-stop search's script, stacks
and launches that test_gpu_forward_edges.py aims at is really in the pool, and the constants of csrc/gki_forward.hip are
the ones the cases were designed for.  Whoever changes one of them learns here that the cases need moving."""
import os
import re
import numpy as np
import pytest

import forward_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _src(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def _facts(name):
    """(k-mers as node lists in all-nodes mode, records in one-node mode) of a pool case"""
    pl = fc.pool()
    i = pl.index[name]
    return fc.kmers_of(pl.results(False)[i]), pl.results(True)[i]


def _ascends(g, start, nodes):
    """the records list a k-mer's nodes by id: the path itself ascends iff that order is a walk from the start node"""
    succ = lambda n: g.edges[g.edge_start[n]:g.edge_start[n + 1]].tolist()
    return nodes[0] == start and all(b in succ(a) for a, b in zip(nodes, nodes[1:]))


def _fits(g, start, kmers):
    """what csrc/gki_forward.hip takes into the script in all-nodes mode: at most FW_SLOTS k-mers, each over at most FW_SN
    nodes with ascending ids"""
    return len(kmers) <= 4 and all(len(p) <= 5 and _ascends(g, start, p) for p in kmers)


def test_the_constants_the_cases_were_designed_for():
    fwd = _src("graph_kmer_index_amd", "csrc", "gki_forward.hip")
    common = _src("graph_kmer_index_amd", "csrc", "gki_common.h")
    api = _src("include", "gki.h")
    assert "constexpr int FW_SLOTS = 4, FW_SN = 5, FW_ENTRY_U4 = 3;" in fwd
    assert re.search(r"constexpr int FWD_BLOCK = 64;", fwd)
    assert "sc.over_cap = n_pos < (1 << 20) ? n_pos : (1 << 20);" in fwd
    assert "static constexpr int64_t LANES = 64 * 256;" in common and 64 * 256 == 16384
    assert re.search(r"#define GKI_MAX_WINDOW_NODES 48\b", api) and "constexpr int FMAX = GKI_MAX_WINDOW_NODES;" in fwd
    # the expansion: four slots of a start position in neighbouring lanes, 256 threads = 64 start positions per block, 16 per wave
    assert "__launch_bounds__(256) void k_forward_expand" in fwd and "const int64_t i = tid / FW_SLOTS;" in fwd
    # the stack edges of test (d): hand-over at L >= cap - 1, the first arena 4 * FMAX levels, doubled from there
    assert "if (L >= cap - 1) { gki_raise(err, GKI_ERR_WINDOW_TOO_DEEP); continue; }" in fwd
    assert fwd.count("gki_deep_next_cap(word[0], da.cap, 4 * FMAX)") == 1 and fwd.count("gki_deep_next_cap(word, da.cap, 4 * FMAX)") == 1
    assert "const int next_cap = cap == 0 ? first_cap : 2 * cap;" in common
    # the successor count of test (f): 16 bits, 0xFFFF = ask edge_start
    assert "w.cnt = (uint16_t)(cnt < 0xFFFF ? cnt : 0xFFFF);" in fwd


def test_every_finished_kmer_count_and_path_length_is_in_the_pool():
    pl = fc.pool()
    all_nodes, one_node = pl.results(False), pl.results(True)
    for name, f in (("Lw2", 1), ("F2", 2), ("F3", 3), ("F4_2x2", 4), ("F4_1x4", 4), ("F5", 5), ("F6_2x3", 6), ("fullest", 4), ("fit3_then6", 4)):
        kmers, one = _facts(name)
        assert len(kmers) == f == len(one["kmers"]), name
        assert len(set(all_nodes[pl.index[name]]["kmers"].tolist())) == f, name           # different paths, different hashes
    for lw in range(2, 8):
        kmers, one = _facts("Lw%d" % lw)
        assert [len(p) for p in kmers] == [lw] and _ascends(pl.graph, pl.nodes[pl.index["Lw%d" % lw]], kmers[0])
        assert one["nodes"].tolist() == [min(kmers[0])]                                   # one-node mode reports the smallest id
    # node lists (a path's nodes but the last) of 2, 3 and 4 entries: two pieces, and piece 2 half and fully used
    assert [len(p) - 1 for p in _facts("F2")[0]] == [2, 2]
    assert [len(p) - 1 for p in _facts("F4_2x2")[0]] == [3] * 4
    assert [len(p) - 1 for p in _facts("fullest")[0]] == [4] * 4 and len(all_nodes[pl.index["fullest"]]["kmers"]) == 20
    # which cases fit the script in all-nodes mode
    fitting = {c.name for c, r, n0 in zip(pl.cases, all_nodes, pl.nodes) if _fits(pl.graph, n0, fc.kmers_of(r))}
    assert fitting == {"Lw2", "Lw3", "Lw4", "Lw5", "F2", "F3", "F4_2x2", "F4_1x4", "fullest", "inside", "dead_end", "dead_allele"}
    # three entries written, then a path that does not fit
    kmers, _ = _facts("fit3_then6")
    assert [len(p) for p in kmers] == [3, 3, 3, 6] and all(_ascends(pl.graph, pl.nodes[pl.index["fit3_then6"]], p) for p in kmers)
    # the fourth fits and the fifth arrives
    assert [len(p) for p in _facts("F5")[0]] == [3] * 5
    # the cheapest overflowing start, and the 1-record and 0-record starts
    kmers, one = _facts("descending")
    i = pl.index["descending"]
    assert len(kmers) == 1 and len(kmers[0]) == 2 and pl.nodes[i] == max(kmers[0]) and not _ascends(pl.graph, pl.nodes[i], kmers[0]) and all_nodes[i]["start_nodes"].tolist() == [min(kmers[0])] * 2
    assert one["nodes"].tolist() == [min(kmers[0])]
    kmers, one = _facts("inside")
    assert kmers == [[int(pl.nodes[pl.index["inside"]])]] and len(one["kmers"]) == 1
    assert all_nodes[pl.index["inside"]]["start_offsets"].tolist() == [pl.offs[pl.index["inside"]] + fc.K - 1]
    for name in ("dead_end", "dead_allele"):
        assert _facts(name)[0] == [] and len(_facts(name)[1]["kmers"]) == 0
    # successors per node on the walked paths: 0, 1, 2, 3, 5 (and 4)
    g = pl.graph
    walked = set(int(n) for r in all_nodes for n in r["nodes"]) | set(int(n) for n in pl.nodes)
    assert {0, 1, 2, 3, 4, 5} <= set(int(g.edge_start[n + 1] - g.edge_start[n]) for n in walked)
    # in one-node mode every case fits but F5 and F6 (the only ones with more than four k-mers)
    assert sorted(c.name for c, r in zip(pl.cases, one_node) if len(r["kmers"]) > 4) == ["F5", "F6_2x3"]
    # allele frequencies: the minimum along the path, and they differ from node to node
    assert len(set(g.allele_freq[sorted(walked)].tolist())) > 20
    for r in all_nodes:
        at = 0
        for p in fc.kmers_of(r):
            assert r["allele_frequencies"][at:at + len(p)].tolist() == [min(g.allele_freq[n] for n in p)] * len(p)
            at += len(p)


@pytest.mark.parametrize("E", [0, 1, 45, 46, 190, 382])
def test_chain(E):
    pl = fc.pool(fc.chain(E))
    r_all, r_one = pl.results(False)[-1], pl.results(True)[-1]
    kmers = fc.kmers_of(r_all)
    assert len(r_all["kmers"]) == E + 2 and len(kmers) == 1 and _ascends(pl.graph, pl.nodes[-1], kmers[0])
    assert len(r_one["kmers"]) == 1 and r_one["nodes"][0] == pl.nodes[-1]
    # the pool beside it is untouched by the extra component
    for a, b in zip(pl.results(False)[:-1], fc.pool().results(False)):
        assert all(np.array_equal(a[key], b[key]) for key in fc.COLS)


@pytest.mark.parametrize("S", [3, 70])
def test_fan(S):
    pl = fc.pool(fc.fan(S))
    kmers = fc.kmers_of(pl.results(False)[-1])
    assert len(kmers) == S and all(len(p) == 3 and _ascends(pl.graph, pl.nodes[-1], p) for p in kmers)
    assert len(set(p[1] for p in kmers)) == S and len(pl.results(True)[-1]["kmers"]) == S
    g, n0 = pl.graph, int(pl.nodes[-1])
    assert g.edge_start[n0 + 1] - g.edge_start[n0] == S


def test_expected_equals_a_plain_loop():
    pl = fc.pool()
    rng = np.random.default_rng(11)
    for one in (False, True):
        nodes, offs, results = pl.with_invalid(one)
        assert len(results) == len(nodes) == len(pl.cases) + 4
        pattern = rng.integers(0, len(results), size=300)
        exp = fc.expected(results, pattern)
        rec_start, cols = [0], {key: [] for key in fc.COLS}
        for p in pattern:
            for key in fc.COLS:
                cols[key] += results[p][key].tolist()
            rec_start.append(rec_start[-1] + len(results[p]["kmers"]))
        assert exp["rec_start"].tolist() == rec_start and exp["rec_start"].dtype == np.int64
        for key, dt in zip(fc.COLS, fc.DTYPES):
            assert exp[key].dtype == dt and exp[key].tolist() == cols[key], key
    empty = fc.expected(results, np.zeros(0, dtype=np.int64))
    assert empty["rec_start"].tolist() == [0] and len(empty["kmers"]) == 0
