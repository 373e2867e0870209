"""Test-side restatement of UniqueVariantKmersFinder's dense path (unique_variant_kmers.py:114-270 of the reference),
rules 1-7 of the port's DESIGN section 4.7, in NumPy over the oracle's early-stop search (oracle.find_from_position)
and a host loop of frequencies.  find_from_position gives no window ids, so a start with more than 500 records (where
the 500-window cap of kmers_found may apply) raises instead of guessing."""
import numpy as np

from oracle import oracle


def start_distances(k):
    return [i for i in range(2, k - 2)][::4][::-1]


def node_at_ref_offset(g, x):
    """(node, offset) of graph ref offset x on the linear path's nonzero-size nodes; ValueError outside."""
    ntro = np.asarray(g.node_to_ref_offset, dtype=np.int64)
    lin = np.nonzero((g.is_ref != 0) & (g.node_size > 0))[0]
    starts = ntro[lin]
    o = np.argsort(starts, kind="stable")
    lin, starts = lin[o], starts[o]
    i = int(np.searchsorted(starts, x, side="right")) - 1
    if i < 0 or x - starts[i] >= g.node_size[lin[i]]:
        raise ValueError("ref offset %d outside the linear path" % x)
    return int(lin[i]), int(x - starts[i])


def unique_variant_kmers(g, ref_nodes, var_nodes, positions, line_numbers, k, max_variant_nodes, frequency,
                         lowest=True, chunk_size=None, chromosome_offsets=None, position_base=None):
    """FlatKmers columns (hashes uint64, nodes uint32, ref_offsets uint64, af float32) of every variant in order.
    frequency: hash -> CollisionFreeKmerIndex.get_frequency(hash) (k=31 reverse complement)."""
    dist = start_distances(k)
    if not dist:
        raise ValueError("no start position for k=%d" % k)
    pb = g.position_id_base() if position_base is None else position_base
    out = []
    found, chunk_of_found = set(), None
    for idx, (pos, line) in enumerate(zip(positions, line_numbers)):
        chunk = idx // chunk_size if chunk_size else 0
        if chunk != chunk_of_found:
            found, chunk_of_found = set(), chunk
        ref, alt = int(ref_nodes[line]), int(var_nodes[line])
        if ref == 0 or alt == 0:
            continue
        store = {n for n in (ref, alt) if n not in found}
        base = 0 if chromosome_offsets is None else chromosome_offsets[idx]
        valid = []
        for j, d in enumerate(dist):
            node, off = node_at_ref_offset(g, base + int(pos) - d)
            rec = oracle.find_from_position(g, k, node, off, False, max_variant_nodes)
            if len(rec["kmers"]) > 500:
                raise NotImplementedError("a start with more than 500 records: the 500-window cap needs window ids")
            h, nd = rec["kmers"], rec["nodes"]
            kref = {int(x) for x, n in zip(h, nd) if n == ref and ref in store}
            kalt = {int(x) for x, n in zip(h, nd) if n == alt and alt in store}
            ok = not (kref & kalt) or j == len(dist) - 1
            if not ok:
                continue
            keep = np.isin(nd, np.array(sorted(store), dtype=np.int64))
            flat = (h[keep].astype(np.uint64), nd[keep].astype(np.uint32),
                    (pb[rec["start_nodes"][keep]] + rec["start_offsets_wide"][keep]).astype(np.uint64),
                    rec["allele_frequencies"][keep].astype(np.float32))
            score = max([0] + [frequency(int(x)) for x in flat[0]])
            valid.append((score, flat))
            if score <= 1:
                break
        if lowest:
            valid = sorted(valid, key=lambda p: p[0])           # stable
        best = valid[0][1]
        found |= {int(n) for n in best[1]}
        out.append(best)
    if not out:
        return (np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.float32))
    return tuple(np.concatenate([f[i] for f in out]) for i in range(4))
