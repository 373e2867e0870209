"""Generate tests/golden/critical_error_order.json by RUNNING THE REFERENCE's CriticalGraphPaths.from_graph on small
graphs that hold BOTH of its errors: a critical point with offset -1 (critical_graph_paths.py:82, failing at :104 once
all walks are done) and a branching node without exactly one linear-ref successor (:96-100, raised inside the walk).

Run in the build container only (needs /root/reference; tests/standins/ replace obgraph):

    python tests/golden/make_golden_critical_errors.py

Stored per case: the graph literals, k, the exception's class name, which error it was, and for the branch error the node
the reference logs ("Did not find 1 next node from node %d") -- data only.  The offset error carries no node in the
reference (numpy refuses the whole array).
"""
import json
import logging
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests", "standins"), "/root/reference", ROOT, os.path.join(ROOT, "tests")]

from graph_kmer_index.critical_graph_paths import CriticalGraphPaths  # noqa: E402
from obgraph import Graph  # noqa: E402

OUT = os.path.join(HERE, "critical_error_order.json")

# offset error: node 1 behind exactly k = 3 bases of single-edge chain; branch error: neither successor is linear-ref
ONE_WALK = ({0: "ACG", 1: "TTTT", 2: "A", 3: "C", 4: "GG"}, {0: [1], 1: [2, 3], 2: [4], 3: [4]}, [0, 1, 4])
TWO_WALKS = ({0: "ACG", 1: "TTTT", 2: "AC", 3: "A", 4: "C", 5: "GG"}, {0: [1], 2: [3, 4], 3: [5], 4: [5]}, [0, 1, 2, 5])
CASES = [("one_walk_offset_then_branch", ONE_WALK, None),
         ("two_walks_offset_then_branch", TWO_WALKS, [0, 2]),
         ("two_walks_branch_then_offset", TWO_WALKS, [2, 0]),
         ("two_walks_offset_alone", TWO_WALKS, [0]),                   # controls: each error on its own
         ("two_walks_branch_alone", TWO_WALKS, [2])]


class _Keep(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.ERROR)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


def main():
    out = []
    for name, (seqs, edges, linear), starts in CASES:
        keep = _Keep()
        logging.getLogger().addHandler(keep)
        try:
            CriticalGraphPaths.from_graph(Graph.from_dicts(seqs, edges, linear, chromosome_start_nodes=starts), 3)
            raised = None
        except Exception as e:          # noqa: BLE001 -- the reference raises a bare Exception / OverflowError
            raised = type(e).__name__
        finally:
            logging.getLogger().removeHandler(keep)
        named = [re.search(r"from node (\d+)", line) for line in keep.lines]
        named = [int(m.group(1)) for m in named if m]
        kind = {"Exception": "branch", "OverflowError": "offset"}[raised]
        assert (kind == "branch") == bool(named)
        out.append({"name": name, "seqs": {str(a): b for a, b in seqs.items()}, "edges": {str(a): b for a, b in edges.items()},
                    "linear": linear, "chromosome_start_nodes": starts, "k": 3, "raises": raised, "kind": kind,
                    "node": named[0] if named else None})
        print("%-32s %-14s %s node=%s" % (name, raised, kind, out[-1]["node"]))
    with open(OUT, "w") as fh:
        json.dump(out, fh, indent=1)
    print("%s: %d bytes" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
