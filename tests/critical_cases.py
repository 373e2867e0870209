"""Graphs that take the device critical-path walk (csrc/gki_critical.hip) off its fast path and past one block (test
utility shared by tests/test_critical_spec.py on the CPU and tests/test_gpu_critical_paths_routes.py on the GPU).

The device has two routes to the path of every chromosome.  THE GUESS -- the linear-ref nodes in id order, checked
against next[] -- holds for every graph built along its genome.  Which route a graph takes cannot be seen from outside
the library, so the cases force it by construction:

  * `relabel(g, perm)` renames node v to perm[v].  Once two consecutive path nodes a -> b carry ids in the wrong order
    the listed node in front of them has next[v] != want (or, when a starts the chromosome, a itself has): the guess
    is rejected and the jump tables run.  `relabellings` gives a random permutation, the ids reversed (every edge leads
    down), only the last two path nodes swapped and only the first two swapped (the start node is no longer the
    chromosome's lowest id);
  * a component that `with_starts` leaves out of the chromosome list still has its linear-ref nodes in the guessed
    slice of the component before it, whose last node then fails "the slice's last node must end the walk".

Everything here is NumPy over whole arrays: the large cases have millions of nodes."""
import functools

import numpy as np

import graphgen
import spec_critical as spec
from graph_kmer_index_amd.graph import GraphArrays, synthetic_indel_graph, synthetic_snp_graph

SCAN_TILE = 2048                      # items per block of the library's scan
GRID_THREADS = 2048 * 256             # threads of the largest grid a streaming kernel gets: more items -> a second round


def _gather_rows(start, order):
    """Rows `order` of a CSR laid out back to back: (new row starts, index into the old flat array)."""
    length = np.diff(start)[order]
    new_start = np.zeros(len(order) + 1, dtype=np.int64)
    np.cumsum(length, out=new_start[1:])
    src = np.repeat(start[:-1][order] - new_start[:-1], length) + np.arange(int(new_start[-1]), dtype=np.int64)
    return new_start, src


def relabel(g, perm):
    """The same graph with node v renamed perm[v] (successor order kept)."""
    perm = np.asarray(perm, dtype=np.int64)
    n = g.n_nodes
    assert perm.shape == (n,) and np.all(np.bincount(perm, minlength=n) == 1)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)                                       # new id u holds the old node inv[u]
    edge_start, e_src = _gather_rows(g.edge_start, inv)
    _, s_src = _gather_rows(g.seq_start, inv)
    ntro = None
    if g.node_to_ref_offset is not None:
        ntro = np.zeros(n + 1, dtype=np.int64)
        ntro[:n] = np.asarray(g.node_to_ref_offset)[:n][inv]
    return GraphArrays(g.node_size[inv], g.seq[s_src], edge_start, perm[g.edges[e_src]].astype(np.int32), g.is_ref[inv],
                       g.allele_freq[inv], g.exists[inv], int(perm[g.first_node]),
                       [int(perm[s]) for s in g.chromosome_start_nodes.values()], ntro)


def concat(graphs):
    """One graph whose chromosomes are the given components, ids and chromosome_start_nodes in the order passed."""
    shift = np.concatenate([[0], np.cumsum([g.n_nodes for g in graphs])]).astype(np.int64)
    e_shift = np.concatenate([[0], np.cumsum([len(g.edges) for g in graphs])]).astype(np.int64)
    edge_start = np.concatenate([g.edge_start[:-1] + e for g, e in zip(graphs, e_shift)] + [e_shift[-1:]])
    edges = np.concatenate([g.edges.astype(np.int64) + s for g, s in zip(graphs, shift)]).astype(np.int32)
    starts = [int(s) + int(sh) for g, sh in zip(graphs, shift) for s in g.chromosome_start_nodes.values()]

    def cat(name):
        return np.concatenate([getattr(g, name) for g in graphs])
    return GraphArrays(cat("node_size"), cat("seq"), edge_start, edges, cat("is_ref"), cat("allele_freq"), cat("exists"),
                       graphs[0].first_node, starts)


def with_starts(g, starts):
    """The same arrays with another chromosome list."""
    return GraphArrays(g.node_size, g.seq, g.edge_start, g.edges, g.is_ref, g.allele_freq, g.exists, g.first_node,
                       [int(s) for s in starts], g.node_to_ref_offset, g.rev_start, g.rev_edges)


def ref_path(g):
    """The walk of a one-chromosome graph built along its genome: its linear-ref(-dummy) nodes in id order (what the
    device guesses).  The last two are checked to end the walk."""
    path = np.flatnonzero(g.is_ref)
    assert path[0] == list(g.chromosome_start_nodes.values())[0]
    assert g.edge_start[path[-1] + 1] == g.edge_start[path[-1]] and path[-1] in g.get_edges(int(path[-2]))
    return path


def swap(n, a, b):
    perm = np.arange(n, dtype=np.int64)
    perm[[a, b]] = perm[[b, a]]
    return perm


def relabellings(n, path, seed=0):
    """name -> permutation; each one takes a graph whose chromosome walks `path` (two nodes or more) off the guess."""
    assert len(path) >= 2
    rng = np.random.default_rng([seed, n])
    random = rng.permutation(n).astype(np.int64)
    a, b = int(path[-2]), int(path[-1])
    if random[a] < random[b]:                                      # make sure of one descending step on the path
        random[[a, b]] = random[[b, a]]
    out = {"random": random, "reversed": np.arange(n - 1, -1, -1, dtype=np.int64), "swap_last": swap(n, a, b)}
    if len(path) >= 3:
        out["swap_first"] = swap(n, int(path[0]), int(path[1]))
    return out


# ------------------------------------------------------------------------------------------------ the small cases
def dicts(seqs, edges, linear, af=None, **kw):
    return GraphArrays.from_dicts(seqs, edges, linear, af, **kw)


def bubble_chain(path_len, seed, max_ref=14):
    """A graphgen SNP/indel chain whose walk has exactly `path_len` nodes: (path_len - 1) // 2 sites of two path nodes
    each behind the first segment, which is split into a single-edge chain of two nodes when path_len is even."""
    rng = np.random.default_rng([seed, path_len])
    chain = {-1: 1} if path_len % 2 == 0 else None
    return dicts(*graphgen.random_bubble_graph(rng, n_var=(path_len - 1) // 2, min_ref=2, max_ref=max_ref, p_indel=0.5,
                                               chain_after=chain))


K_SMALL = 5
SCAN_EDGE_LENGTHS = (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, 2 * SCAN_TILE + 1)                       # (a)
FILL_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 1025)                                              # (b)


@functools.lru_cache(maxsize=None)
def scan_edge_graph(path_len):
    return bubble_chain(path_len, 1)


@functools.lru_cache(maxsize=None)
def fill_components():
    return tuple(bubble_chain(length, 2) for length in FILL_LENGTHS)


def block_relabel(components, which, perm_of):
    """concat(components) with only component `which` relabelled inside its own id range."""
    shift = np.concatenate([[0], np.cumsum([c.n_nodes for c in components])])
    perm = np.arange(int(shift[-1]), dtype=np.int64)
    perm[shift[which]:shift[which + 1]] = shift[which] + perm_of(components[which].n_nodes)
    return relabel(concat(list(components)), perm)


@functools.lru_cache(maxsize=None)
def three_components():
    return tuple(bubble_chain(length, 3) for length in (9, 12, 7))


@functools.lru_cache(maxsize=None)
def many_chromosomes(count):
    return concat([bubble_chain(1 + i % 6, 4 + i) for i in range(count)])                              # (d)


STATE_SEED = 2024                                                                                       # (e)
STATE_GRAPHS = 300


def state_graphs():
    """(e): (index, k, graph as built, a random permutation, the graph under it) for 300 random graphs that open depth
    above 2 (nested, deep_nested, overlapping), carry single-edge chains of k - 1, k and k + 1 bases behind a join,
    and empty nodes."""
    rng = np.random.default_rng(STATE_SEED)
    for it in range(STATE_GRAPHS):
        k = int(rng.integers(2, 13))
        kind = it % 4
        if kind == 0:
            chain = {int(rng.integers(0, 3)): k - 1 + int(rng.integers(0, 3))}
            lit = graphgen.random_bubble_graph(rng, n_var=int(rng.integers(3, 9)), min_ref=k + 2, max_ref=2 * k + 4,
                                               p_indel=0.6, chain_after=chain)
        elif kind == 1:
            lit = graphgen.nested_bubble_graph(rng, n_var=int(rng.integers(2, 7)), min_ref=1, max_ref=12, p_nest=0.6, p_chain=0.4)
        elif kind == 2:
            lit = graphgen.deep_nested_graph(rng, n_var=int(rng.integers(1, 5)), max_depth=3)
        else:
            lit = graphgen.overlapping_bubble_graph(rng)
        g = dicts(*lit[:3])
        perm = rng.permutation(g.n_nodes)
        yield it, k, g, perm, relabel(g, perm)


def cycle_graph():
    """(h): 0 -> 1 -> 2 -> {1, 3}: node 2 branches, its one linear-ref successor is node 1 again."""
    return dicts({0: "ACGT", 1: "AC", 2: "GT", 3: "TT"}, {0: [1], 1: [2], 2: [1, 3]}, [0, 1, 2])


# ------------------------------------------------------------------------------------------------ the large cases
K_LARGE = 31
SECOND_ROUND_SITES = 270_000          # (f): three nodes a site, two of them on the path
THREE_LEVEL_SITES = 2_110_000         # (g): the path has more than 2048 * 2048 + 2048 nodes


@functools.lru_cache(maxsize=None)
def second_round_graph():
    g = synthetic_indel_graph(60 * SECOND_ROUND_SITES, SECOND_ROUND_SITES, k=K_LARGE, seed=61, p_del=0.15, p_ins=0.15)
    assert g.n_nodes > GRID_THREADS and len(ref_path(g)) > GRID_THREADS
    return g


@functools.lru_cache(maxsize=None)
def three_level_graph():
    g = synthetic_snp_graph(16 * THREE_LEVEL_SITES, int(THREE_LEVEL_SITES * 1.16), k=K_LARGE, seed=62)
    assert len(ref_path(g)) > SCAN_TILE * SCAN_TILE + SCAN_TILE
    return g


def offset_error_component(k=K_LARGE):
    """Node 1 is reached after exactly k bases of single-edge chain: offset -1."""
    return dicts({0: "A" * k, 1: "TTTT"}, {0: [1]}, [0, 1]), 1


def branch_error_component():
    """Node 1 branches into two nodes neither of which is linear-ref; it is the component's last linear-ref node, so the
    guessed slice ends on it and the guess itself stands."""
    return dicts({0: "ACGTACGT", 1: "AC", 2: "A", 3: "C", 4: "GG"}, {0: [1], 1: [2, 3], 2: [4], 3: [4]}, [0, 1]), 1


def error_precedence_cases(big):
    """name -> (graph, kind, node): the large graph with both errors behind it in either order, and with the offset error
    alone."""
    (off, off_node), (branch, branch_node) = offset_error_component(), branch_error_component()
    n = big.n_nodes
    return {"offset_then_branch": (concat([big, off, branch]), "branch", n + off.n_nodes + branch_node),
            "branch_then_offset": (concat([big, branch, off]), "branch", n + branch_node),
            "offset_alone": (concat([big, off]), "offset", n + off_node)}


# ------------------------------------------------------------------------------------------------ reading the library
def library_outcome(g, k, on_device):
    """CriticalGraphPaths.from_graph as one comparable value, like spec_critical.outcome: (nodes, offsets) as lists --
    dtypes checked -- or ("raises", kind, node named in the message); a cycle names no node."""
    import re
    from graph_kmer_index_amd import CriticalGraphPaths
    try:
        cp = CriticalGraphPaths.from_graph(g, k, on_device=on_device)
    except Exception as e:          # noqa: BLE001 -- the reference raises a bare Exception / OverflowError here
        text = str(e)
        kind = "offset" if "offset -1" in text else "branch" if "linear-ref successor" in text else \
            "cycle" if "found a cycle" in text else text
        named = re.search(r"node (\d+)", text)
        return ("raises", kind, int(named.group(1)) if named and kind != "cycle" else None)
    assert cp.nodes.dtype == np.uint32 and cp.offsets.dtype == np.uint16
    return cp.nodes.tolist(), cp.offsets.tolist()


def same_outcome(got, want):
    """a cycle names no node in the library's message"""
    if want[0] == "raises" and want[1] == "cycle":
        return got[:2] == want[:2]
    return got == want


def renamed(outcome, perm):
    """What an outcome on g becomes on relabel(g, perm): nodes renamed, order and offsets kept."""
    if outcome[0] == "raises":
        return outcome[:2] + (None if outcome[2] is None else int(perm[outcome[2]]),)
    return perm[np.asarray(outcome[0], dtype=np.int64)].tolist(), outcome[1]


def check_against_spec(g, k, outcome_of, perms=None, want_values=True):
    """`outcome_of(g, k)` (the host walk in the CPU tests, the device in the GPU tests) equals the spec on g as built and
    under every relabelling, where the spec itself obeys result(relabel(g, p)).nodes == p[result(g).nodes] with equal
    offsets.  Returns the spec's outcome on g."""
    want = spec.outcome(g, k)
    assert same_outcome(outcome_of(g, k), want)
    if want_values:
        assert want[0] != "raises" and len(want[0]) > 0
    for name, p in (perms or {}).items():
        moved = relabel(g, p)
        want_moved = spec.outcome(moved, k)
        assert want_moved == renamed(want, p), name
        assert same_outcome(outcome_of(moved, k), want_moved), name
    return want


def longest_path(g, k):
    return max(spec.walk(g, k)[0], key=len)
