"""The early-stop search (csrc/gki_forward.hip: gki_forward_count / gki_forward_emit) at the capacities of its script, of
the script's expansion, of the overflow list, of its stacks and of its launches, on the designed graphs of
tests/forward_cases.py (test_forward_cases_host.py proves from the oracle that the cases are what they are named for).

Every call makes the same three comparisons (forward_cases.assert_call), exact in values, dtypes and record order: the
emit that expands the script against the emit that walks, the first against the oracle's records laid out for the call,
and the count and rec_start against the same.  No tolerance: the allele-frequency column is a minimum of inputs.  Both
sets of output columns are filled with 0xA5 and are 64 records longer than the count says: the guard must stay, the fill
inside must go."""
import numpy as np
import pytest

import forward_cases as fc

pytestmark = pytest.mark.gpu
MODES = [pytest.param(False, id="all_nodes"), pytest.param(True, id="one_node")]


class OnDevice:
    """a Pool and its DeviceGraph"""

    def __init__(self, pl):
        from graph_kmer_index_amd.device_graph import DeviceGraph
        self.pool, self.dev = pl, DeviceGraph(pl.graph)

    def check(self, one, pattern, nodes=None, offs=None, results=None):
        """one call with start position i = case pattern[i] (of the pool, or of nodes / offs / results)"""
        pattern = np.asarray(pattern, dtype=np.int64)
        nodes, offs = (self.pool.nodes, self.pool.offs) if nodes is None else (nodes, offs)
        got = fc.run_both(self.dev, fc.K, fc.M, one, nodes[pattern], offs[pattern])
        fc.assert_call(self.pool.results(one) if results is None else results, pattern, got)
        return got

    def close(self):
        self.dev.close()


@pytest.fixture(scope="module")
def shallow():
    d = OnDevice(fc.pool())
    yield d
    d.close()


def _idx(pl, *names):
    return [pl.index[n] for n in names]


# ------------------------------------------------------------------------------------------------ a. script capacity
@pytest.mark.parametrize("one", MODES)
def test_script_capacity(shallow, one):
    """forward_walk, `fits = used < FW_SLOTS && (one_node || (short_path && asc))`, and script_write / k_forward_expand's
    pairing of piece 2 (written when `listed > 2`, read when `lw > 3`): every pool case alone (n_pos = 1) and all of them in
    one call -- 1 to 6 finished k-mers, paths of 2 to 7 nodes, node lists of 1 to 4 entries, the start that writes three
    entries and then meets a path of six nodes (`used = 0xFF`: skipped whole by the expansion, filled by the walk), the fifth
    k-mer arriving at a full script, the window inside the start node (`have0 == k`), the starts without a record.  In
    one-node mode the paths of six and seven nodes fit (`one_node ||`) and report the smallest node id."""
    pl = shallow.pool
    for i in range(len(pl.cases)):
        shallow.check(one, [i])
    got = shallow.check(one, np.arange(len(pl.cases)))
    per_start = np.diff(got["rec_start"])
    assert per_start[pl.index["fullest"]] == (4 if one else 20) and per_start[pl.index["Lw7"]] == (1 if one else 7)


# ------------------------------------------------------------------------------------------------ b. expansion geometry
def _patterns(pl, n_pos, n_with_invalid):
    i = np.arange(n_pos)
    fullest, f4, f5, fit3, desc, dead, inside, f6 = _idx(pl, "fullest", "F4_2x2", "F5", "fit3_then6", "descending", "dead_end", "inside", "F6_2x3")
    none_or_over = np.array([dead, f5, desc, f6])
    yield "every wave full", np.full(n_pos, fullest)
    yield "a wave without a scripted record between two full ones", np.where((i // 16) % 3 == 1, none_or_over[i % 4], fullest)
    yield "scripted and walked alternate", np.where(i % 2 == 0, f4, f5)
    edge = np.where(i % 16 == 15, fullest, np.where(i % 16 == 0, f5, np.array([inside, fit3, f4])[i % 3]))
    yield "a wave's last scripted, the next one's first walked", edge
    yield "a wave's last walked, the next one's first scripted", np.where(i % 16 == 15, f5, np.where(i % 16 == 0, fullest, edge))
    yield "the pool and the invalid starts, stride 7", (i * 7) % n_with_invalid


@pytest.mark.parametrize("one", MODES)
@pytest.mark.parametrize("n_pos", [15, 16, 17, 63, 64, 65, 255, 256, 257, 1025])
def test_expansion_geometry(shallow, one, n_pos):
    """k_forward_expand: `i = tid / FW_SLOTS` (16 start positions per wave, 64 per block), the wave's prefix sum
    (`gki_wave_incl_sum`, `excl_slot0`), the rounds `for (rr0 = 0; rr0 < R; rr0 += 64)` -- sixteen fullest starts are 320
    records, five rounds -- the binary search over `s_ex` across lanes without records, and `if (i < n_pos)` in the last,
    partial wave; with it the walking kernel's list (`EMIT && list ? list[t] : t`) for the starts in between.  Start
    positions that are not in the graph (node id -1, node id n_nodes: `n0 < 0 || n0 >= g.n_nodes`; offset -1, offset
    node_size + 1: `o0 < 0 || o0 > w0.size`) give no record and leave their neighbours' alone."""
    pl = shallow.pool
    nodes, offs, results = pl.with_invalid(one)
    for what, pattern in _patterns(pl, n_pos, len(nodes)):
        shallow.check(one, pattern, nodes, offs, results)


def _at_end(d, one):
    """every case's start node at offset == node_size, between the pool's own starts"""
    from oracle import oracle
    pl = d.pool
    at_end = pl.graph.node_size[pl.nodes].astype(np.int32)
    extra = [oracle.find_from_position(pl.graph, fc.K, int(n), int(o), one, fc.M) for n, o in zip(pl.nodes, at_end)]
    nodes, offs = np.concatenate([pl.nodes, pl.nodes]), np.concatenate([pl.offs, at_end])
    return nodes, offs, pl.results(one) + extra


@pytest.mark.parametrize("one", MODES)
def test_offset_equal_to_node_size(shallow, one):
    """forward_walk, `if (o0 < 0 || o0 > w0.size)` and `outside0 = o0 == w0.size && w0.size > 0`: a start at offset ==
    node_size is taken, with no base of the start node.  The oracle defines it as the reference does: search_from's loop over
    the node's bases does not run, the successors are searched with an empty path, and the start node is NOT among the
    window's nodes -- it is in no record, its allele frequency is not in the minimum, it is not the smallest node id of
    one-node mode.  (Before this test the walk counted the start node in: one record too many per k-mer in all-nodes mode,
    the wrong node in one-node mode.)  Every pool case's start node at that offset between the pool's own starts, 80 and
    1025 start positions; then the same beside chain(60), where the deep variant walks them (levels 1 .. L by selection)."""
    nodes, offs, results = _at_end(shallow, one)
    n_pool = len(shallow.pool.cases)
    assert sum(len(r["kmers"]) for r in results[n_pool:]) > 20
    i5 = shallow.pool.index["F5"]                 # five k-mers of two nodes each: start node left out, (allele, join) remain
    assert len(results[n_pool + i5]["kmers"]) == (5 if one else 10) and shallow.pool.nodes[i5] not in results[n_pool + i5]["nodes"]
    for n_pos in (80, 1025):
        shallow.check(one, (np.arange(n_pos) * 7) % len(nodes), nodes, offs, results)
    d = OnDevice(fc.pool(fc.chain(60)))
    try:
        nodes, offs, results = _at_end(d, one)
        assert len(results[-1]["kmers"]) == (1 if one else 61)
        d.check(one, (np.arange(80) * 7) % len(nodes), nodes, offs, results)
        d.check(one, [len(nodes) - 1], nodes, offs, results)
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ c. overflow list
LIST_CAP = 1 << 20


@pytest.mark.parametrize("n_pos, n_over, one, over", [
    pytest.param(LIST_CAP + 4096, LIST_CAP, False, "descending", id="list_exactly_full"),
    pytest.param(LIST_CAP + 4096, LIST_CAP + 1, False, "descending", id="unlisted"),
    pytest.param(LIST_CAP + 4096, LIST_CAP + 1, True, "F5", id="unlisted_one_node"),
    pytest.param(300, 300, False, "descending", id="small_list_full"),
])
def test_overflow_list(shallow, n_pos, n_over, one, over):
    """gki_forward_emit, `listed = sc.overflow <= sc.over_cap` with `over_cap = min(n_pos, 2^20)`: the list exactly full
    (2^20 of 2^20 + 4096 starts overflow; 300 of 300), and one more than it holds -- then k_forward<EMIT> gets no list and
    one lane per start position, and `if (EMIT && used && !list && used[i] != 0xFF) continue;` skips the scripted ones; in
    the count pass `if (slot < list_n) list[slot] = i` drops the entry that does not fit.  The starts that fit (the window
    inside the start node, 1 record) lie 257 positions apart, so they take every lane of a wave in turn; there are 4096 of
    them among 16 448 blocks of 64, so not every block can have one.  Expected records: forward_cases.expected(), index
    arithmetic only."""
    pl = shallow.pool
    pattern = np.full(n_pos, pl.index[over])
    pattern[(np.arange(n_pos - n_over) * 257) % n_pos] = pl.index["inside"]
    assert int(np.sum(pattern == pl.index[over])) == n_over
    got = shallow.check(one, pattern)
    assert got["n"] == n_over * (5 if one else 2) + (n_pos - n_over)


# ------------------------------------------------------------------------------------------------ d. stack edges
@pytest.mark.parametrize("one", MODES)
@pytest.mark.parametrize("lo, hi", [(40, 52), (184, 196), (378, 390)])
def test_stack_edges(one, lo, hi):
    """forward_walk, `if (L >= cap - 1) gki_raise(err, GKI_ERR_WINDOW_TOO_DEEP)`, and gki_deep_next_cap(word, da.cap, 4 * FMAX)
    in both entry points.  chain(E) is a start node, E empty nodes and the node that completes the k-mer; the walk holds
    E + 1 levels when it meets the last, so with cap levels a chain fits while E + 1 < cap - 1.  The product kernel
    (cap = FMAX = 48) answers up to E = 45 and E = 46 is the first to move the call to the deep variant; its first arena
    (192 levels) answers up to E = 189, E = 190 is the first to need 384 levels and E = 382 the first to need 768.  Every E of
    40..52, 184..196 and 378..390, with a fitting start before the chain and an overflowing one behind it: the count call
    climbs from the product kernel, and so does each emit call on its own (gki_forward_emit ends with deep_release)."""
    for E in range(lo, hi + 1):
        d = OnDevice(fc.pool(fc.chain(E)))
        try:
            pl = d.pool
            got = d.check(one, [pl.index["fullest"], pl.index["chain%d" % E], pl.index["F5"]])
            assert np.diff(got["rec_start"])[1] == (1 if one else E + 2)
        finally:
            d.close()


# ------------------------------------------------------------------------------------------------ e. deep grid stride
@pytest.mark.parametrize("one", MODES)
def test_deep_grid_stride(one):
    """k_forward<.., DEEP>, `for (t = lane_global; t < n_items; t += DEEP ? da.lanes : n_items)`: the deep variant's 16 384
    lanes (DeepArenaOwner::LANES) walk 16 384 + 70 start positions, so 70 lanes go round twice and walk a second start
    on the levels of the first.  chain(60) -- too deep for the product kernel, see test_stack_edges -- at positions 3,
    16 383, 16 384 and the last moves the whole call there; the shallow pool is cycled everywhere else."""
    d = OnDevice(fc.pool(fc.chain(60)))
    try:
        pl = d.pool
        n_pos = 16384 + 70
        pattern = (np.arange(n_pos) * 7) % (len(pl.cases) - 1)
        pattern[[3, 16383, 16384, n_pos - 1]] = pl.index["chain60"]
        got = d.check(one, pattern)
        assert np.diff(got["rec_start"])[[3, 16383, 16384, n_pos - 1]].tolist() == [1 if one else 62] * 4
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ f. successor counts
@pytest.mark.parametrize("one", MODES)
@pytest.mark.parametrize("S", [3, 65534, 65535, 65536])
def test_successor_counts(one, S):
    """k_build_fwd, `w.cnt = (uint16_t)(cnt < 0xFFFF ? cnt : 0xFFFF)`, and succ_begin's last line: three or more successors
    index g.edges from `w.e0` to `w.e0 + w.cnt`, or to `g.edge_start[n + 1]` when the count reads 0xFFFF -- 65 534 is the
    largest count the record holds itself, 65 535 and 65 536 ask edge_start.  fan(S): S one-base successors of the start
    node that join one node, S k-mers of three nodes (S = 3 fits the script, the others are walked).  One start per call,
    and the start 65 times (a second wave)."""
    d = OnDevice(fc.Pool([fc.fan(S)]))
    try:
        for n_pos in (1, 65):
            got = d.check(one, np.zeros(n_pos, dtype=np.int64))
            assert got["n"] == n_pos * S * (1 if one else 3)
    finally:
        d.close()
