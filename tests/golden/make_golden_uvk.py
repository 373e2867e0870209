"""Generate tests/golden/uvk_reference.json.gz by RUNNING THE REFERENCE's UniqueVariantKmersFinder (dense path).

Run in the build container only (needs /root/reference; tests/standins/ replace obgraph and friends):

    python tests/golden/make_golden_uvk.py

The stand-in obgraph Graph has no positional accessors; the subclass below adds them as the port assumes them
(graph ref offset = node_to_ref_offset[chromosome start] + offset; the node at a ref offset is the
linear-ref node of nonzero size that covers it).  The frequency index is the reference's CollisionFreeKmerIndex of a
flat made from the graph's own k-mers (one node per k-mer, hashes with hash % 3 == 0 dropped so that frequencies 0, 1
and more occur); it is stored as (hash, number of distinct ref offsets) pairs, which is all get_frequency reads.  `-c` chunks are made the way
the CLI makes them: one finder per chunk of variant lines.  Stored: graph dicts, variants, variant-to-nodes, the
index's k-mer frequencies, the parameters and the output columns -- data only.
"""
import gzip
import json
import logging
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests", "standins"), "/root/reference", ROOT, os.path.join(ROOT, "tests")]
logging.disable(logging.CRITICAL)

import numpy as np  # noqa: E402
from obgraph import Graph  # noqa: E402
from obgraph.position_id import PositionId  # noqa: E402
from graph_kmer_index.kmer_finder import DenseKmerFinder  # noqa: E402
from graph_kmer_index.flat_kmers import FlatKmers  # noqa: E402
from graph_kmer_index.collision_free_kmer_index import CollisionFreeKmerIndex  # noqa: E402
from graph_kmer_index.unique_variant_kmers import UniqueVariantKmersFinder  # noqa: E402

from uvk_cases import planted_chromosome, planted_graph  # noqa: E402

OUT = os.path.join(HERE, "uvk_reference.json.gz")


class PositionalGraph(Graph):
    def _lin(self):
        lin = [n for n in self._linear_list if len(self._seq[n])]
        return lin, np.array([self.node_to_ref_offset[n] for n in lin], dtype=np.int64)

    def convert_chromosome_ref_offset_to_graph_ref_offset(self, offset, chromosome):
        return int(self.node_to_ref_offset[self.chromosome_start_nodes[chromosome]]) + int(offset)

    def get_node_at_ref_offset(self, x):
        lin, st = self._lin()
        return lin[int(np.searchsorted(st, x, side="right")) - 1]

    def get_node_offset_at_ref_offset(self, x):
        return int(x) - int(self.node_to_ref_offset[self.get_node_at_ref_offset(x)])


class _Variant:
    def __init__(self, position, chromosome, line):
        self.position, self.chromosome, self.vcf_line_number = position, chromosome, line


class _V2N:
    def __init__(self, ref, var):
        self.ref_nodes, self.var_nodes = np.asarray(ref), np.asarray(var)


def make_case(name, seed, chromosomes, k=31, m=6, lowest=True, chunk_size=None, extra=None):
    rng = np.random.default_rng(seed)
    chroms = [planted_chromosome(rng, **c) for c in chromosomes]
    ns, ed, lin, starts, variants = planted_graph(chroms)
    g = PositionalGraph(ns, ed, lin, chromosome_start_nodes=starts)
    pid = PositionId.from_graph(g)
    f = DenseKmerFinder(g, k, max_variant_nodes=4, position_id=pid, only_save_one_node_per_kmer=True)
    f.find()
    fl = f.get_flat_kmers(v="1")
    hashes = np.asarray(fl._hashes, dtype=np.int64)
    refs = np.asarray(fl._ref_offsets, dtype=np.int64)
    keep = hashes % 3 != 0
    hashes, refs = hashes[keep], refs[keep]
    z = np.zeros(len(hashes), np.int64)
    index = CollisionFreeKmerIndex.from_flat_kmers(FlatKmers(hashes, z, refs, z.astype(float)), modulo=10007)
    # get_frequency reads the number of distinct ref offsets of a k-mer (collision_free_kmer_index.py:267-293)
    pairs = np.unique(np.stack([hashes, refs]), axis=1)
    uh, cnt = np.unique(pairs[0], return_counts=True)
    # variant lines: every site, then (extra) lines that reuse nodes of earlier ones; line 1 holds node 0 (skipped)
    rows = [(p, c, r, a) for p, c, r, a in variants]
    if extra == "shared":
        rows = [x for pair in zip(rows, rows) for x in pair]       # split multi-allelic lines sharing both nodes
    rows.insert(1, (rows[0][0], rows[0][1], 0, rows[0][3]))
    ref = [r for _, _, r, _ in rows]
    var = [a for _, _, _, a in rows]
    vs = [_Variant(p, c, i) for i, (p, c, _, _) in enumerate(rows)]
    chunks = [vs] if chunk_size is None else [vs[i:i + chunk_size] for i in range(0, len(vs), chunk_size)]
    flats = []
    for chunk in chunks:
        u = UniqueVariantKmersFinder(g, _V2N(ref, var), chunk, k, m, kmer_index_with_frequencies=index,
                                     do_not_choose_lowest_frequency_kmers=not lowest, use_dense_kmer_finder=True,
                                     position_id_index=pid)
        flats.append(u.find_unique_kmers())
    out = FlatKmers.from_multiple_flat_kmers(flats)
    return {"name": name, "seed": seed, "k": k, "max_variant_nodes": m, "lowest": lowest, "chunk_size": chunk_size,
            "graph": {"node_sequences": {str(n): s for n, s in ns.items()}, "edges": {str(n): e for n, e in ed.items()},
                      "linear_ref_nodes": lin, "chromosome_start_nodes": starts},
            "variants": {"positions": [p for p, _, _, _ in rows], "chromosomes": [c for _, c, _, _ in rows],
                         "lines": list(range(len(rows)))},
            "ref_nodes": ref, "var_nodes": var,
            "index": {"modulo": 10007, "hashes": [int(x) for x in uh], "counts": [int(x) for x in cnt]},
            "expected": {"hashes": [int(x) for x in out._hashes], "nodes": [int(x) for x in out._nodes],
                         "ref_offsets": [int(x) for x in out._ref_offsets],
                         "allele_frequencies": [float(x) for x in out._allele_frequencies]}}


def main():
    base = dict(length=4000, n_snps=25, n_dels=3, n_repeats=8)
    cases = []
    for lowest in (True, False):
        tag = "lowest" if lowest else "first"
        cases.append(make_case("snp_del_repeats_%s" % tag, 11, [base], lowest=lowest))
        cases.append(make_case("k15_%s" % tag, 12, [base], k=15, lowest=lowest))
        cases.append(make_case("m3_%s" % tag, 13, [base], m=3, lowest=lowest))
        cases.append(make_case("two_chromosomes_%s" % tag, 14, [dict(base, length=2500), dict(base, length=2500)],
                               lowest=lowest))
    for cs in (None, 2, 5):
        cases.append(make_case("shared_nodes_chunk_%s" % cs, 15, [dict(base, n_snps=12)], chunk_size=cs,
                               extra="shared"))
    cases.append(make_case("over_500_windows", 16, [dict(length=600, n_snps=2, cluster=10)]))
    with gzip.open(OUT, "wt") as fh:
        json.dump({"cases": cases}, fh)
    print("%s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
