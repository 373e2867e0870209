"""The rules of DESIGN.md 4.19 (include/gki.h, "haplotype paths") as plain Python: a haplotype's sequence by walking the
graph's edges, its alt nodes by a loop over the lines, its node counts by hashing the spelled strings and looking every
hash up in the index's host arrays.  No device and nothing of graph_kmer_index_amd.haplotype_paths: this is the oracle of
tests/test_gpu_haplotype_paths.py, itself checked in tests/test_haplotype_paths_spec.py."""
import numpy as np

import read_side_ref

LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)


def takes_alt(code):
    """Slot code -> whether the slot takes the alt allele: 1 only; 0, 2 (another allele) and 3 (none) follow the ref."""
    return int(code) == 1


def seq_start_of(graph):
    return np.concatenate([[0], np.cumsum(np.asarray(graph.node_size), dtype=np.int64)])


def spell(graph, ref_nodes, var_nodes, codes, slot, chromosome_start_nodes):
    """The letters (uint8 arrays, upper-case ACGT) of slot `slot`, one array per chromosome: from the chromosome's start
    node along `edges`; a node with two successors stands before a kept line's two allele nodes and the slot's code of
    that line chooses between them.  codes: uint8[V][H]."""
    seq_start = seq_start_of(graph)
    line_of = {}
    for v in range(len(var_nodes)):
        if int(var_nodes[v]) != 0:
            line_of[(int(ref_nodes[v]), int(var_nodes[v]))] = v
    out = []
    for start in chromosome_start_nodes:
        pieces, n = [], int(start)
        while True:
            pieces.append(np.asarray(graph.seq[seq_start[n]:seq_start[n + 1]]))
            succ = [int(x) for x in graph.edges[graph.edge_start[n]:graph.edge_start[n + 1]]]
            if not succ:
                break
            if len(succ) == 1:
                n = succ[0]
                continue
            assert len(succ) == 2, "node %d has %d successors" % (n, len(succ))
            v = line_of.get((succ[0], succ[1]), line_of.get((succ[1], succ[0])))
            assert v is not None, "the successors %s of node %d are no kept line's allele nodes" % (succ, n)
            n = int(var_nodes[v]) if takes_alt(codes[v][slot]) else int(ref_nodes[v])
        codes_of_path = np.concatenate(pieces) if pieces else np.zeros(0, np.uint8)
        out.append(LETTERS[codes_of_path])
    return out


def alt_nodes(var_nodes, codes, slot):
    """var_nodes[v] of the kept lines v at which the slot takes the alt allele, in line order."""
    out = []
    for v in range(len(var_nodes)):
        if int(var_nodes[v]) != 0 and takes_alt(codes[v][slot]):
            out.append(int(var_nodes[v]))
    return np.array(out, dtype=np.uint32)


def index_arrays(index):
    """A CollisionFreeKmerIndex's host arrays as the dict tests/read_side_ref.py probes."""
    return {"_kmers": np.asarray(index._kmers), "_nodes": np.asarray(index._nodes), "_frequencies": None,
            "_modulo": int(index._modulo)}


def node_counts(strings, index, k, n_nodes, include_reverse_complement=True):
    """Node hit counts (uint32[n_nodes]) of all k-mers of `strings` (one uint8 array per chromosome; none across a
    boundary) and, when asked for, of their reverse complements."""
    letters = np.concatenate(strings) if strings else np.zeros(0, np.uint8)
    read_start = np.concatenate([[0], np.cumsum([len(s) for s in strings])]).astype(np.int64)
    arrays = index_arrays(index)
    counts = np.zeros(n_nodes, dtype=np.int64)
    for strand in (0, 1) if include_reverse_complement else (0,):
        hashes, _ = read_side_ref.hash_reads_ref(letters, read_start, k, strand)
        # every distinct hash is looked up once and its hits count as often as the hash occurs (at k = 5 a hash occurs
        # hundreds of times and has hundreds of hits); the products stay far below 2^53, so float64 weights are exact
        distinct, times = np.unique(hashes, return_counts=True)
        _, positions, query = read_side_ref.probe_ref(arrays, distinct, 2 ** 62)
        nodes = arrays["_nodes"][positions].astype(np.int64)
        inside = nodes < n_nodes
        counts += np.rint(np.bincount(nodes[inside], weights=times[query][inside], minlength=n_nodes)).astype(np.int64)
    return counts.astype(np.uint32)
