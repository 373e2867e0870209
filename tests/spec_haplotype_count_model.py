"""The rules of DESIGN.md 4.20 (include/gki.h, "haplotype segments" and "node count model") as plain Python loops: the
taken lines' intervals by walking the graph's edges, the segments by the rule's own formula, the dirty windows by brute
force, window counts over a k-mer -> nodes table, and the count model.  No device and nothing of
graph_kmer_index_amd.haplotype_paths: this is the oracle of tests/test_gpu_haplotype_count_model.py, itself checked in
tests/test_haplotype_count_model_spec.py."""
import numpy as np

from spec_haplotype_paths import seq_start_of, takes_alt

COMPLEMENT = {65: 84, 67: 71, 71: 67, 84: 65}              # A <-> T, C <-> G


def walk(graph, ref_nodes, var_nodes, codes, slot, chromosome_start_nodes, along_slot):
    """The sequence that slot `slot` (along_slot) or the all-ref path (not along_slot) spells, walked along the edges:
    (bounds, intervals).  bounds[c] is where chromosome c begins, bounds[-1] the length.  intervals holds, for every line
    slot `slot` takes the alt allele of, in line order, (chromosome, a, b): where the allele of that line which the walked
    sequence goes through lies in it -- the alt allele along the slot, the ref allele along the all-ref path."""
    seq_start = seq_start_of(graph)
    line_of = {}
    for v in range(len(var_nodes)):
        if int(var_nodes[v]) != 0:
            line_of[(int(ref_nodes[v]), int(var_nodes[v]))] = v
    bounds, intervals, at = [0], [], 0
    for c, start in enumerate(chromosome_start_nodes):
        n = int(start)
        while True:
            at += int(seq_start[n + 1] - seq_start[n])
            succ = [int(x) for x in graph.edges[graph.edge_start[n]:graph.edge_start[n + 1]]]
            if not succ:
                break
            if len(succ) == 1:
                n = succ[0]
                continue
            v = line_of.get((succ[0], succ[1]), line_of.get((succ[1], succ[0])))
            taken = takes_alt(codes[v][slot])
            n = int(var_nodes[v]) if taken and along_slot else int(ref_nodes[v])
            if taken:
                intervals.append((c, at, at + int(seq_start[n + 1] - seq_start[n])))
        bounds.append(at)
    return bounds, intervals


def segments(bounds, intervals, k):
    """The rule's runs: [(start, windows)] in line order, empty runs left out."""
    out, b_prev = [], 0
    for c, a, b in intervals:
        lo = max(a - k + 1, b_prev, bounds[c])
        hi = min(b - 1, bounds[c + 1] - k)
        if hi >= lo:
            out.append((lo, hi - lo + 1))
        b_prev = b
    return out


def dirty_windows(bounds, intervals, k):
    """By brute force: every window start of every chromosome that is dirty for some taken line's interval."""
    out = []
    for c in range(len(bounds) - 1):
        for s in range(bounds[c], bounds[c + 1] - k + 1):
            if any(s < b and a < s + k for _, a, b in intervals):
                out.append(s)
    return out


def window_starts(segs):
    return [s for start, n in segs for s in range(start, start + n)]


def reverse_complement(window):
    return bytes(COMPLEMENT[x] for x in reversed(window))


def count_windows(letters, starts, table, k, n_nodes, include_reverse_complement=True):
    """int64[n_nodes]: for every window start in `starts` the nodes `table` (bytes -> list of nodes) holds for the window's
    letters and, when asked for, for its reverse complement."""
    counts = np.zeros(n_nodes, dtype=np.int64)
    text = bytes(bytearray(letters))
    for s in starts:
        w = text[s:s + k]
        assert len(w) == k
        for key in (w, reverse_complement(w)) if include_reverse_complement else (w,):
            for node in table.get(key, ()):
                if node < n_nodes:
                    counts[node] += 1
    return counts


def all_window_starts(bounds, k):
    return [s for c in range(len(bounds) - 1) for s in range(bounds[c], bounds[c + 1] - k + 1)]


def model(rows, codes, ref_nodes, var_nodes, samples, ploidy, n_bins):
    """(histogram uint32[V][2][ploidy + 1][n_bins], count_sum uint64[V][2][ploidy + 1]) of the individuals `samples`,
    rows[i] (one count per node) the row of samples[i], sample s owning the slots s * ploidy .. s * ploidy + ploidy - 1."""
    v_lines = len(var_nodes)
    histogram = np.zeros((v_lines, 2, ploidy + 1, n_bins), dtype=np.uint32)
    count_sum = np.zeros((v_lines, 2, ploidy + 1), dtype=np.uint64)
    for row, s in zip(rows, samples):
        for v in range(v_lines):
            if int(var_nodes[v]) == 0:
                continue
            c_alt = sum(1 for h in range(s * ploidy, s * ploidy + ploidy) if takes_alt(codes[v][h]))
            for allele, node, copies in ((0, int(ref_nodes[v]), ploidy - c_alt), (1, int(var_nodes[v]), c_alt)):
                count = int(row[node]) if node < len(row) else 0
                histogram[v][allele][copies][min(count, n_bins - 1)] += 1
                count_sum[v][allele][copies] += np.uint64(count)
    return histogram, count_sum
