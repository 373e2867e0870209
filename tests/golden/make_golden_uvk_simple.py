"""Generate tests/golden/uvk_simple_reference.json.gz by RUNNING THE REFERENCE's UniqueVariantKmersFinder with
use_simple=True (find_kmers_over_variant, unique_variant_kmers.py:66-111).

Run in the build container only (needs the reference checkout; tests/standins/ replace obgraph and friends):

    python tests/golden/make_golden_uvk_simple.py

The stand-in obgraph Graph has no positional accessors; the subclass below adds the six this mode calls, as the port
assumes them.  get_node_sequence is only compared with "" by the reference, so any string of the node's
length serves.  Stored: graph dicts, variants with their types, variant-to-nodes, the parameters and the output columns --
data only.
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
from graph_kmer_index.unique_variant_kmers import UniqueVariantKmersFinder  # noqa: E402

from uvk_simple_cases import GOLDEN, random_sites, sites_graph  # noqa: E402


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

    def get_node_sequence(self, node):
        return "x" * len(self._seq[node])

    def get_node_at_chromosome_and_chromosome_offset(self, chromosome, offset):
        return self.get_node_at_ref_offset(self.convert_chromosome_ref_offset_to_graph_ref_offset(offset, chromosome))

    def get_node_offset_at_chromosome_and_chromosome_offset(self, chromosome, offset):
        return self.get_node_offset_at_ref_offset(self.convert_chromosome_ref_offset_to_graph_ref_offset(offset, chromosome))


class _Variant:
    def __init__(self, position, chromosome, line, is_snp):
        self.position, self.chromosome, self.vcf_line_number = position, chromosome, line
        self.type = "SNP" if is_snp else "INDEL"


class _V2N:
    def __init__(self, ref, var):
        self.ref_nodes, self.var_nodes = np.asarray(ref), np.asarray(var)


def make_case(name, seed, k, m, gap, n_chromosomes=1, length=3000, n_sites=60, shared=False):
    rng = np.random.default_rng(seed)
    chroms = [random_sites(rng, length, n_sites, gap[0], gap[1] + 1) for _ in range(n_chromosomes)]
    ns, ed, lin, starts, rows = sites_graph(chroms)
    if shared:                       # every fifth site on two lines (split multi-allelic lines): its records come twice
        rows = [r for i, r in enumerate(rows) for _ in range(2 if i % 5 == 0 else 1)]
    rows.insert(1, (rows[0][0], rows[0][1], 0, rows[0][3], rows[0][4]))              # a line with ref node 0: skipped
    g = PositionalGraph(ns, ed, lin, chromosome_start_nodes=starts)
    ref, var = [r[2] for r in rows], [r[3] for r in rows]
    vs = [_Variant(r[0], r[1], i, r[4]) for i, r in enumerate(rows)]
    out = UniqueVariantKmersFinder(g, _V2N(ref, var), vs, k, m, use_simple=True,
                                   position_id_index=PositionId.from_graph(g)).find_unique_kmers()
    return {"name": name, "seed": seed, "k": k, "max_variant_nodes": m,
            "graph": {"node_sequences": {str(n): s for n, s in ns.items()}, "edges": {str(n): e for n, e in ed.items()},
                      "linear_ref_nodes": lin, "chromosome_start_nodes": starts},
            "variants": {"positions": [r[0] for r in rows], "chromosomes": [r[1] for r in rows],
                         "lines": list(range(len(rows))), "is_snp": [r[4] for r in rows]},
            "ref_nodes": ref, "var_nodes": var,
            "expected": {"hashes": [int(x) for x in out._hashes], "nodes": [int(x) for x in out._nodes],
                         "ref_offsets": [int(x) for x in out._ref_offsets],
                         "allele_frequencies": [float(x) for x in out._allele_frequencies]}}


def main():
    cases = [make_case("k31_m6_sparse", 21, 31, 6, (40, 80)),
             make_case("k31_m6_dense", 22, 31, 6, (3, 12)),
             make_case("k15_m6_dense", 23, 15, 6, (3, 12)),
             make_case("k31_m2_dense", 26, 31, 2, (2, 8)),
             make_case("k5_m6", 25, 5, 6, (10, 30)),
             make_case("k31_m0_dense", 30, 31, 0, (3, 12)),
             make_case("two_chromosomes", 27, 31, 6, (3, 40), n_chromosomes=2, length=1500, n_sites=30),
             make_case("shared_nodes", 28, 31, 6, (3, 40), length=1500, n_sites=30, shared=True)]
    with gzip.open(GOLDEN, "wt") as fh:
        json.dump({"cases": cases}, fh)
    print("%s: %d cases, %d bytes" % (GOLDEN, len(cases), os.path.getsize(GOLDEN)))
    for c in cases:
        print(c["name"], len(c["expected"]["hashes"]))


if __name__ == "__main__":
    main()
