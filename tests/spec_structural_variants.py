"""Test-side restatement of sample_kmers_from_structural_variants (structural_variants.py:6-43 of the reference) in
NumPy, rules 1-8 of DESIGN section 4.9.  The frequency source is a table (sorted distinct hashes, the first hit's
frequency of each): get_frequency(h) = table[h] + table[rc31(h)], the reverse complement taken at k = 31 whatever k is.
Also the reader of tests/golden/sv_kmers_reference.json.gz (tests/golden/make_golden_sv_kmers.py: the reference's own
output)."""
import gzip
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_M = np.uint64


def window_hashes(codes, k):
    """hash of every window of a numeric sequence: sum_i base[j + i] * 4^i (uint64[len - k + 1])."""
    codes = np.asarray(codes).astype(np.uint64)
    if len(codes) < k:
        return np.zeros(0, np.uint64)
    w = np.lib.stride_tricks.sliding_window_view(codes, k)
    return (w << (2 * np.arange(k)).astype(np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)


def revcomp(h, k):
    """reverse complement of k-mer hashes at k <= 31: complement every 2-bit digit, reverse the digit order."""
    x = ~np.asarray(h, dtype=np.uint64) & _M((1 << (2 * k)) - 1)
    x = ((x >> _M(2)) & _M(0x3333333333333333)) | ((x & _M(0x3333333333333333)) << _M(2))
    x = ((x >> _M(4)) & _M(0x0F0F0F0F0F0F0F0F)) | ((x & _M(0x0F0F0F0F0F0F0F0F)) << _M(4))
    return x.byteswap() >> _M(64 - 2 * k)


class FrequencyTable:
    def __init__(self, hashes, frequencies):
        h = np.asarray(hashes, dtype=np.uint64)
        o = np.argsort(h, kind="stable")
        self.hashes, self.frequencies = h[o], np.asarray(frequencies, dtype=np.int64)[o]
        assert len(np.unique(self.hashes)) == len(self.hashes)

    @classmethod
    def from_index(cls, index):
        """From a CollisionFreeKmerIndex' host arrays: the frequency of the first record of every k-mer (the records of
        a bucket lie together, in bucket order)."""
        kmers, first = np.unique(np.asarray(index._kmers).astype(np.uint64), return_index=True)
        return cls(kmers, np.asarray(index._frequencies)[first])

    def first_hit(self, q):
        q = np.asarray(q, dtype=np.uint64)
        if len(self.hashes) == 0:
            return np.zeros(len(q), np.int64)
        i = np.minimum(np.searchsorted(self.hashes, q), len(self.hashes) - 1)
        return np.where(self.hashes[i] == q, self.frequencies[i], 0)

    def get_frequency(self, h, rc_k=31):
        return self.first_hit(h) + self.first_hit(revcomp(h, rc_k))


def valid_windows(g, node, table, k, max_frequency, rc_k=31):
    """(hashes of all windows of the node, ascending valid window offsets)."""
    h = window_hashes(g.get_numeric_node_sequence(node), k)
    return h, np.nonzero(table.get_frequency(h, rc_k) < max_frequency)[0]


def greedy(valid, k):
    chosen, prev = [], -10000
    valid = np.asarray(valid, dtype=np.int64)
    while True:
        i = int(np.searchsorted(valid, prev + k))            # the first valid window at or after prev + k
        if i == len(valid):
            return np.array(chosen, dtype=np.int64)
        prev = int(valid[i])
        chosen.append(prev)


def sample_kmers(g, pairs, table, k, max_frequency=2, rc_k=31):
    """(hashes uint64, nodes uint32, ref_offsets uint32) in the reference's order.  rc_k is 31 in the reference; another
    value shows what its quirk changes."""
    hashes, nodes = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint32)]
    for node in np.asarray(pairs, dtype=np.int64).reshape(-1).tolist():
        if g.get_node_size(node) > k + 5:
            h, valid = valid_windows(g, node, table, k, max_frequency, rc_k)
            chosen = greedy(valid, k)
            hashes.append(h[chosen])
            nodes.append(np.full(len(chosen), node, dtype=np.uint32))
    hashes, nodes = np.concatenate(hashes), np.concatenate(nodes)
    return hashes, nodes, np.zeros(len(hashes), dtype=np.uint32)


# ------------------------------------------------------------------ the fixture
def load_cases():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "sv_kmers_reference.json.gz"), "rt") as fh:
        return json.load(fh)["cases"]


def case_graph(case):
    from graph_kmer_index_amd.graph import GraphArrays
    gr = case["graph"]
    return GraphArrays.from_dicts({int(n): s for n, s in gr["node_sequences"].items()},
                                  {int(n): e for n, e in gr["edges"].items()}, gr["linear_ref_nodes"])


def case_table(case):
    return FrequencyTable(case["index"]["hashes"], case["index"]["counts"])


def case_index_flat(case):
    """A flat whose index has the stored frequencies: `count` records of each hash at distinct ref offsets."""
    from graph_kmer_index_amd.flat_kmers import FlatKmers
    counts = np.array(case["index"]["counts"], dtype=np.int64)
    h = np.repeat(np.array(case["index"]["hashes"], dtype=np.uint64), counts)
    first = np.repeat(np.cumsum(counts) - counts, counts)
    refs = (np.arange(len(h)) - first).astype(np.uint64)
    z = np.zeros(len(h), np.uint32)
    return FlatKmers(h, z, refs, z.astype(np.float32))


def expected(case):
    e = case["expected"]
    return tuple(np.array(e[key], dtype=np.dtype(e["dtypes"][key]))
                 for key in ("hashes", "nodes", "ref_offsets", "allele_frequencies"))
