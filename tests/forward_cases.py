"""Designed graphs for the early-stop search (csrc/gki_forward.hip) and what its two emit forms must write.

A CASE is a small graph and one start position (node, offset), built for one property of the count pass's script, of its
expansion or of the walk: how many k-mers finish (F), how many nodes a path has (Lw), how many successors a node has.
Every case of a pool lives in ONE graph as a disjoint component with an id offset of its own, so that one call can mix
them in any pattern.  The expected records of a call come from the oracle, once per case, and are laid out for a
pattern of cases with index arithmetic (expected()): the big calls have over 10^6 start positions.

Used by test_forward_cases_host.py (a census of the pool from the oracle alone, no GPU) and test_gpu_forward_edges.py."""
import ctypes as C
import numpy as np

from graph_kmer_index_amd.graph import GraphArrays
from oracle import oracle

K, M = 7, 4
COLS = ("kmers", "start_nodes", "start_offsets", "nodes", "allele_frequencies")
DTYPES = (np.int64, np.int32, np.int16, np.int32, np.float64)
FILL, GUARD = 0xA5, 64
HEAD, TAIL = "GATTACAGAT", "TGCATGCATG"             # a start node and a node that completes the k-mer (>= K bases)
ALLELES = {1: ["A", "C", "G", "T"], 2: ["AC", "CG", "GT", "TA", "AA", "CC"]}      # distinct bases per allele of one site


class Case:
    def __init__(self, name, seqs, edges, lin, start, offset, prop):
        self.name, self.seqs, self.edges, self.lin, self.start, self.offset, self.prop = name, seqs, edges, lin, start, offset, prop

    def __repr__(self):
        return self.name


def layered(name, sites, prop, take=1):
    """Start node 0, then one layer of nodes per site (every allele of a site leads to every allele of the next, in list
    order; the first allele of a site is the linear-ref one), then TAIL.  The start offset leaves as many bases of the
    start node as make the window complete `take` bases into TAIL; a path has len(sites) + 2 nodes."""
    width = sum(len(s[0]) for s in sites)
    r = K - take - width
    assert 1 <= r <= len(HEAD) and 1 <= take <= len(TAIL) and all(len(set(map(len, s))) == 1 and len(set(s)) == len(s) for s in sites)
    seqs, edges, lin = {0: HEAD}, {}, [0]
    prev, nxt = [0], 1
    for s in sites:
        ids = list(range(nxt, nxt + len(s)))
        for i, a in zip(ids, s):
            seqs[i] = a
        for p in prev:
            edges[p] = ids
        lin.append(ids[0])
        prev, nxt = ids, nxt + len(s)
    seqs[nxt] = TAIL
    for p in prev:
        edges[p] = [nxt]
    lin.append(nxt)
    return Case(name, seqs, edges, lin, 0, len(HEAD) - r, prop)


def site(n):
    return ALLELES[1 if n <= 4 else 2][:n]


def singles(n):
    return [["ACGTA"[d]] for d in range(n)]


def pool_cases():
    """The pool: every case with the property it is built for (test_forward_cases_host.py asserts each from the oracle)."""
    cases = [layered("Lw%d" % (n + 2), singles(n), "one path over %d nodes" % (n + 2)) for n in range(6)]       # Lw2 .. Lw7; Lw2 is F = 1
    cases += [
        layered("F2", [site(2)], "two k-mers of three nodes: node lists of two"),
        layered("F3", [site(3)], "three k-mers; a node with three successors"),
        layered("F4_2x2", [site(2), ["G", "T"]], "four k-mers as two consecutive SNP sites: node lists of three (piece 2)"),
        layered("F4_1x4", [site(4)], "four k-mers from one four-allele site: the script exactly full"),
        layered("F5", [site(5)], "the fourth path fits and a fifth arrives; a node with five successors"),
        layered("F6_2x3", [site(2), site(3)], "six k-mers as 2 x 3"),
        layered("fullest", [site(2), ["G"], ["T", "A"]], "four fitting paths of five nodes: 20 records, node lists of four", take=2),
    ]
    # three paths of three nodes fit, the fourth has six nodes: the whole start is walked
    seqs = {0: HEAD, 1: "A", 2: "C", 3: "G", 4: "T", 5: "A", 6: "C", 7: "G", 8: TAIL}
    edges = {0: [1, 2, 3, 4], 1: [8], 2: [8], 3: [8], 4: [5], 5: [6], 6: [7], 7: [8]}
    cases.append(Case("fit3_then6", seqs, edges, [0, 1, 5, 6, 7, 8], 0, len(HEAD) - 2, "three entries written, then a path of six nodes"))
    # the start node's id is above its successor's: the cheapest start that does not fit (all-nodes mode)
    cases.append(Case("descending", {0: TAIL, 1: HEAD}, {1: [0]}, [1, 0], 1, len(HEAD) - 3, "a path of two nodes whose ids descend"))
    cases.append(Case("inside", {0: HEAD + "TACA"}, {}, [0], 0, 2, "the window is complete inside the start node: one record"))
    cases.append(Case("dead_end", {0: HEAD[:6]}, {}, [0], 0, 2, "no successor before k bases: no record"))
    cases.append(Case("dead_allele", {0: HEAD, 1: "A"}, {0: [1]}, [0, 1], 0, len(HEAD) - 3, "one successor, then a dead end: no record"))
    return cases


def chain(E):
    """A start node, then E empty nodes with one successor each, then TAIL: one path over E + 2 nodes."""
    seqs = {0: HEAD, E + 1: TAIL}
    seqs.update({i: "" for i in range(1, E + 1)})
    return Case("chain%d" % E, seqs, {i: [i + 1] for i in range(E + 1)}, list(range(E + 2)), 0, len(HEAD) - (K - 1),
                "one path over %d nodes" % (E + 2))


def fan(S):
    """A start node with S one-base successors that all join TAIL: S k-mers of three nodes each."""
    seqs = {0: HEAD, S + 1: TAIL}
    seqs.update({i: "ACGT"[(i - 1) % 4] for i in range(1, S + 1)})
    edges = {i: [S + 1] for i in range(1, S + 1)}
    edges[0] = list(range(1, S + 1))
    return Case("fan%d" % S, seqs, edges, [0, 1, S + 1], 0, len(HEAD) - (K - 2), "a node with %d successors" % S)


class Pool:
    """The cases as disjoint components of one graph, ids shifted per case; allele frequencies differ from node to node
    (dyadic, so the minimum along a path is exact)."""

    def __init__(self, cases):
        self.cases = list(cases)
        self.index = {c.name: i for i, c in enumerate(self.cases)}
        seqs, edges, lin, shift = {}, {}, [], 0
        self.nodes, self.offs = np.zeros(len(self.cases), np.int32), np.zeros(len(self.cases), np.int32)
        for i, c in enumerate(self.cases):
            seqs.update({n + shift: s for n, s in c.seqs.items()})
            edges.update({n + shift: [m + shift for m in e] for n, e in c.edges.items()})
            lin += [n + shift for n in c.lin]
            self.nodes[i], self.offs[i] = c.start + shift, c.offset
            shift += max(c.seqs) + 1
        af = {n: ((n * 37) % 97 + 1) / 128.0 for n in seqs}
        self.graph = GraphArrays.from_dicts(seqs, edges, lin, af)
        self._results = {}

    def results(self, one):
        """The oracle's columns per case (computed once per mode; callers must not change them)."""
        one = bool(one)
        if one not in self._results:
            self._results[one] = [oracle.find_from_position(self.graph, K, int(n), int(o), one, M) for n, o in zip(self.nodes, self.offs)]
        return self._results[one]

    def with_invalid(self, one):
        """(nodes, offs, results) of the pool followed by four start positions that are not in the graph -- node id -1, node
        id n_nodes, offset -1, offset node_size + 1 -- which give no record."""
        g = self.graph
        first = int(self.nodes[0])
        nodes = np.concatenate([self.nodes, np.array([-1, g.n_nodes, first, first], np.int32)])
        offs = np.concatenate([self.offs, np.array([0, 0, -1, int(g.node_size[first]) + 1], np.int32)])
        empty = {key: np.zeros(0, dt) for key, dt in zip(COLS, DTYPES)}
        return nodes, offs, self.results(one) + [empty] * 4


_POOLS = {}


def pool(extra=None):
    """The pool's graph, alone or with one further case (a chain or a fan) as its last component."""
    key = None if extra is None else extra.name
    if key not in _POOLS:
        _POOLS[key] = Pool(pool_cases() + ([] if extra is None else [extra]))
    return _POOLS[key]


def kmers_of(res):
    """All-nodes records grouped into k-mers (runs of equal hash and end position): a list of node lists."""
    out, prev = [], None
    for h, sn, so, n in zip(res["kmers"].tolist(), res["start_nodes"].tolist(), res["start_offsets"].tolist(), res["nodes"].tolist()):
        if (h, sn, so) != prev:
            out.append([])
            prev = (h, sn, so)
        out[-1].append(n)
    return out


def expected(pool_results, pattern):
    """The five columns and rec_start of a call whose start position i is case pattern[i].  Index arithmetic only."""
    pattern = np.asarray(pattern, dtype=np.int64)
    n_of = np.array([len(r["kmers"]) for r in pool_results], dtype=np.int64)
    base = np.concatenate([[0], np.cumsum(n_of)])[:-1]                  # first record of a case in the concatenated pool
    counts = n_of[pattern]
    rec_start = np.zeros(len(pattern) + 1, dtype=np.int64)
    np.cumsum(counts, out=rec_start[1:])
    total = int(rec_start[-1])
    start_of = np.repeat(np.arange(len(pattern), dtype=np.int64), counts)
    src = base[pattern[start_of]] + (np.arange(total, dtype=np.int64) - rec_start[start_of])
    out = {key: np.concatenate([np.asarray(r[key], dtype=dt) for r in pool_results]).astype(dt, copy=False)[src] for key, dt in zip(COLS, DTYPES)}
    out["rec_start"] = rec_start
    return out


def run_both(graph, k, M, one, nodes, offs):
    """gki_forward_count, then gki_forward_emit twice with the same arguments on a DeviceGraph: the first emit expands the
    count pass's script, the second finds none and walks.  Both sets of output columns are allocated GUARD records longer
    than the count says and filled with the byte FILL first.  Returns n, rec_start and both sets of columns (host arrays of
    n + GUARD records); check_fill() asserts on the guard and on the fill."""
    from graph_kmer_index_amd import _lib
    lib = _lib.load()
    nodes, offs = np.ascontiguousarray(nodes, dtype=np.int32), np.ascontiguousarray(offs, dtype=np.int32)
    held = []
    try:
        d_nodes, d_offs = _lib.DeviceArray.from_host(nodes), _lib.DeviceArray.from_host(offs)
        d_start = _lib.DeviceArray(len(nodes) + 1, np.int64)
        held += [d_nodes, d_offs, d_start]
        n = C.c_int64(0)
        args = (graph.handle, k, M, int(bool(one)), None, d_nodes.ptr, d_offs.ptr, len(nodes))
        _lib.check(lib.gki_forward_count(*args, d_start.ptr, C.byref(n)))
        sets = []
        for emit in range(2):
            cols = [_lib.DeviceArray(n.value + GUARD, d) for d in DTYPES]
            held += cols
            for c in cols:
                _lib.check(lib.gki_memset(c.ptr, FILL, c.nbytes))
            _lib.check(lib.gki_forward_emit(*args, d_start.ptr, *[c.ptr for c in cols]))
            sets.append([c.to_host() for c in cols])
            for c in cols:
                c.free()
        return dict(n=n.value, rec_start=d_start.to_host(), first=sets[0], second=sets[1])
    finally:
        for x in held:
            x.free()


def check_fill(cols, n):
    """The GUARD records behind the n that were asked for are untouched, and no record inside n kept the fill (no column
    of a record can hold it: it is negative as a node id, an offset and a frequency, and wider than 2k bits as a hash)."""
    for c, dt in zip(cols, DTYPES):
        size = np.dtype(dt).itemsize
        assert c.dtype == dt and len(c) == n + GUARD
        assert np.all(c[n:].view(np.uint8) == FILL), "a record was written past the %d the count pass announced" % n
        assert not np.any(c[:n].view("u%d" % size) == int.from_bytes(bytes([FILL]) * size, "little")), "a record was left unwritten"


def assert_call(pl_results, pattern, got):
    """The three comparisons of every test: script emit == walking emit, script emit == expected(), count and rec_start ==
    expected(); exact, values and dtypes, in record order."""
    exp = expected(pl_results, pattern)
    n = int(exp["rec_start"][-1])
    assert got["n"] == n
    assert got["rec_start"].dtype == np.int64 and np.array_equal(got["rec_start"], exp["rec_start"])
    check_fill(got["first"], n)
    check_fill(got["second"], n)
    for key, a, b in zip(COLS, got["first"], got["second"]):
        assert a.dtype == b.dtype == exp[key].dtype, key
        assert np.array_equal(a[:n].view(np.uint8), b[:n].view(np.uint8)), "column %s: the script's expansion differs from the walk" % key
        assert np.array_equal(a[:n].view(np.uint8), exp[key].view(np.uint8)), "column %s differs from the oracle" % key
