"""Simple selection restated as a loop of the oracle's early-stop search (unique_variant_kmers.py:66-111, 241-269 of the
reference): for every variant in order, skipped when its ref or alt node is 0, one search for the ref node and one for the
alt node with only_store_nodes = only_follow_nodes = {node}."""
import numpy as np

from oracle import oracle
from spec_unique_variant_kmers import node_at_ref_offset


def search_start(g, node, position, is_snp, chromosome_offset=0):
    """(start node, start offset) of the search for `node` of a variant at 1-based POS `position`."""
    if is_snp and g.node_size[node] > 0:
        return int(node), 0
    p = position if not is_snp else position - 1                 # 0-based chromosome offset (:72-77)
    return node_at_ref_offset(g, chromosome_offset + p - 8)


def searches(g, ref_nodes, var_nodes, positions, line_numbers, is_snp, chromosome_offsets=None):
    """[(variant index, target node, start node, start offset)] in output order."""
    out = []
    for idx, (pos, line) in enumerate(zip(positions, line_numbers)):
        ref, alt = int(ref_nodes[line]), int(var_nodes[line])
        if ref == 0 or alt == 0:
            continue
        co = 0 if chromosome_offsets is None else int(chromosome_offsets[idx])
        for node in (ref, alt):
            out.append((idx, node) + search_start(g, node, int(pos), bool(is_snp[idx]), co))
    return out


def columns(records, position_base):
    """FlatKmers columns of oracle records (get_flat_kmers(v="1")): uint64, uint32, uint64, float32."""
    cat = lambda key, dt: np.concatenate([r[key] for r in records]).astype(dt) if records else np.zeros(0, dt)
    sn, so = cat("start_nodes", np.int64), cat("start_offsets_wide", np.int64)
    return (cat("kmers", np.int64).view(np.uint64), cat("nodes", np.uint32), (position_base[sn] + so).astype(np.uint64),
            cat("allele_frequencies", np.float32))


def simple_variant_kmers(g, ref_nodes, var_nodes, positions, line_numbers, is_snp, k, max_variant_nodes,
                         chromosome_offsets=None, position_base=None, follow="node"):
    """follow: "node" = the search's own node (the mode itself); None = no only_follow_nodes; a set = that one set for
    every search (what a batch-wide follow mask would do)."""
    pb = g.position_id_base() if position_base is None else np.asarray(position_base, dtype=np.int64)
    recs = []
    for _, node, sn, so in searches(g, ref_nodes, var_nodes, positions, line_numbers, is_snp, chromosome_offsets):
        f = {node} if follow == "node" else follow
        recs.append(oracle.find_from_position(g, k, sn, so, False, max_variant_nodes, only_store_nodes={node},
                                              only_follow_nodes=f))
    return columns(recs, pb)
