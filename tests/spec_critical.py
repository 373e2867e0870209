"""CriticalGraphPaths.from_graph (critical_graph_paths.py:42-104) restated line by line over `GraphArrays` (test utility).

It shares no code with the oracle (oracle/gki_oracle.c) or the library: a plain Python walk over lists.  Where the
reference raises, `SpecError(kind, node)` says why and where, in the reference's order:

  "branch"  a branching node of the walk without exactly one linear-ref successor -- raised INSIDE the walk (:96-100),
            so it beats every offset error, wherever either sits and in whichever chromosome;
  "offset"  a critical point after exactly k bases of single-edge chain has offset -1, which only fails when the offsets
            become uint16 AFTER all walks (:104); `node` is the first such point met;
  "cycle"   the reference would never return: the walk took more than n_nodes + 1 steps (or left the graph).
"""
import numpy as np


class SpecError(Exception):
    def __init__(self, kind, node):
        super().__init__("%s error at node %d" % (kind, node))
        self.kind = kind
        self.node = int(node)


def walk(g, k):
    """(path of every chromosome, nodes, offsets) with offsets as plain ints (-1 kept); raises "branch" and "cycle"."""
    size = g.node_size.tolist()
    e_start, edges = g.edge_start.tolist(), g.edges.tolist()
    in_deg = np.diff(g.rev_start).tolist()
    is_ref = g.is_ref.tolist()
    n = g.n_nodes
    paths, nodes, offsets = [], [], []
    for start in g.chromosome_start_nodes.values():                      # :53
        cur, depth, bp, steps = int(start), 0, 0, 0
        path = []
        while True:
            steps += 1
            if cur < 0 or cur >= n or steps > n + 1:
                raise SpecError("cycle", cur)
            path.append(cur)
            prev_depth = depth
            depth -= in_deg[cur]                                         # :67
            if prev_depth > 1 and depth == 0:                            # :68-70
                bp = 0
            node_size = size[cur]
            if depth == 0 and node_size != 0:                            # :76
                if bp <= k and bp + node_size >= k:                      # :78
                    nodes.append(cur)
                    offsets.append(k - bp - 1)                           # :82
            nxt = edges[e_start[cur]:e_start[cur + 1]]                   # :85
            depth += len(nxt)
            if len(nxt) == 0:
                break
            if len(nxt) == 1:
                bp += node_size                                          # :91
                cur = nxt[0]
            else:
                nxt = [m for m in nxt if is_ref[m]]                      # :95
                if len(nxt) != 1:
                    raise SpecError("branch", cur)                       # :96-100
                cur = nxt[0]
        paths.append(path)
    return paths, nodes, offsets


def critical_paths(g, k):
    """(nodes uint32, offsets uint16) in the reference's order, or SpecError."""
    _, nodes, offsets = walk(g, k)
    for node, off in zip(nodes, offsets):                                # :104 np.array(..., np.uint16)
        if off < 0:
            raise SpecError("offset", node)
    return np.array(nodes, dtype=np.uint32), np.array(offsets, dtype=np.uint16)


def outcome(g, k):
    """(nodes list, offsets list) or ("raises", kind, node): one comparable value."""
    try:
        nodes, offsets = critical_paths(g, k)
    except SpecError as e:
        return ("raises", e.kind, e.node)
    return nodes.tolist(), offsets.tolist()
