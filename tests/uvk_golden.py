"""Cases of tests/golden/uvk_reference.json.gz (tests/golden/make_golden_uvk.py: the reference's own output)."""
import gzip
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_cases():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "uvk_reference.json.gz"), "rt") as fh:
        return json.load(fh)["cases"]


def case_graph(case):
    from graph_kmer_index_amd.graph import GraphArrays
    gr = case["graph"]
    return GraphArrays.from_dicts({int(n): s for n, s in gr["node_sequences"].items()},
                                  {int(n): e for n, e in gr["edges"].items()}, gr["linear_ref_nodes"],
                                  chromosome_start_nodes=gr["chromosome_start_nodes"])


def case_counts(case):
    return dict(zip(case["index"]["hashes"], case["index"]["counts"]))


def case_index_flat(case):
    from graph_kmer_index_amd.flat_kmers import FlatKmers
    """A flat whose index has the stored frequencies: `count` records of each hash at distinct ref offsets."""
    counts = np.array(case["index"]["counts"], dtype=np.int64)
    h = np.repeat(np.array(case["index"]["hashes"], dtype=np.uint64), counts)
    first = np.repeat(np.cumsum(counts) - counts, counts)
    refs = (np.arange(len(h)) - first).astype(np.uint64)
    z = np.zeros(len(h), np.uint32)
    return FlatKmers(h, z, refs, z.astype(np.float32))


def rc31(h):
    from graph_kmer_index_amd.kmer_hashing import kmer_hash_to_reverse_complement_hash
    return int(kmer_hash_to_reverse_complement_hash(int(h), 31))


def case_frequency(case):
    counts = case_counts(case)
    return lambda h: counts.get(int(h), 0) + counts.get(rc31(h), 0)


def expected(case):
    e = case["expected"]
    return (np.array(e["hashes"], dtype=np.uint64), np.array(e["nodes"], dtype=np.uint32),
            np.array(e["ref_offsets"], dtype=np.uint64), np.array(e["allele_frequencies"], dtype=np.float32))


def chromosome_offsets(case, g):
    starts = case["graph"]["chromosome_start_nodes"]
    ntro = np.asarray(g.node_to_ref_offset)
    return [int(ntro[starts[c - 1]]) for c in case["variants"]["chromosomes"]]
