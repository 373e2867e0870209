"""Generate tests/golden/sv_kmers_reference.json.gz by RUNNING THE REFERENCE's sample_kmers_from_structural_variants.

Run in the build container only (needs /root/reference; tests/standins/ replace obgraph and friends):

    python tests/golden/make_golden_sv_kmers.py

The reference's module imports bionumpy for its window hashes; bionumpy is not available, so a stub module stands in for
the import and `bionumpy_hash` is replaced by the reference's own ReadKmers.get_kmers_from_read_dynamic(seq,
power_array(k)), fed the node's letters, (the reference's test pins bionumpy_hash to sequence_to_kmer_hash, the same hash).  The frequency index
is the reference's CollisionFreeKmerIndex of a flat with `count` records of each planted hash at distinct ref offsets;
it is stored as (hash, count) pairs, which is all get_frequency reads.  Stored: graph dicts, the (ref, var) pairs, the
index's k-mer frequencies, k, max_frequency and the output columns with their dtypes -- data only.

Every case plants features (tests/test_structural_variants_spec.py asserts on the stored data that each is hit):
sizes k+5 / k+6, a node whose every window is frequent, frequencies that only the reverse complement contributes, k = 15
where the reverse complement at k = 31 changes the result, max_frequency 1 / 2 / 5, valid windows at j, j+k-1, j+k, a
node under two variants, ref == var, node 0 entries, a node of more than 64 * 64 windows, empty input.
"""
import gzip
import json
import logging
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests", "standins"), "/root/reference", ROOT, os.path.join(ROOT, "tests")]
logging.disable(logging.CRITICAL)
sys.modules.setdefault("bionumpy", types.ModuleType("bionumpy"))

import numpy as np  # noqa: E402
from obgraph import Graph  # noqa: E402
from graph_kmer_index import structural_variants as ref_sv  # noqa: E402
from graph_kmer_index.collision_free_kmer_index import CollisionFreeKmerIndex  # noqa: E402
from graph_kmer_index.flat_kmers import FlatKmers, numeric_to_letter_sequence  # noqa: E402
from graph_kmer_index.kmer_hashing import power_array  # noqa: E402
from graph_kmer_index.read_kmers import ReadKmers  # noqa: E402

import spec_structural_variants as spec  # noqa: E402

# get_kmers_from_read_dynamic takes letters (its letter_sequence_to_numeric maps a numeric array to zeros), so the node's
# numeric sequence goes through the reference's own numeric_to_letter_sequence first
ref_sv.bionumpy_hash = lambda seq, k: ReadKmers.get_kmers_from_read_dynamic(numeric_to_letter_sequence(np.asarray(seq)),
                                                                            power_array(k))

OUT = os.path.join(HERE, "sv_kmers_reference.json.gz")
_CODE = {"a": 0, "c": 1, "g": 2, "t": 3}


def rand_seq(rng, n):
    return "".join(rng.choice(list("acgt"), n)) if n else ""


def bubble_graph(rng, bubbles):
    """Node 0 is the empty "no node"; then segment, (ref allele, alt allele), segment, ...: bubble b has ref node 3b + 2
    and alt node 3b + 3."""
    ns, ed, lin = {0: ""}, {}, []
    nid = 1
    for ref_len, alt_len in bubbles:
        ns[nid], ns[nid + 1], ns[nid + 2] = rand_seq(rng, int(rng.integers(5, 50))), rand_seq(rng, ref_len), rand_seq(rng, alt_len)
        ed[nid] = [nid + 1, nid + 2]
        ed[nid + 1] = [nid + 3]
        ed[nid + 2] = [nid + 3]
        lin += [nid, nid + 1]
        nid += 3
    ns[nid] = rand_seq(rng, 20)
    lin.append(nid)
    return ns, ed, lin


def hashes_of(ns, node, k):
    return spec.window_hashes(np.array([_CODE[c] for c in ns[node]], dtype=np.uint8), k)


class Planter:
    """The (hash -> count) table of a case.  A later assignment of a hash wins."""

    def __init__(self):
        self.counts = {}

    def set(self, h, count):
        if count > 0:
            self.counts[int(h)] = int(count)
        else:
            self.counts.pop(int(h), None)

    def table(self):
        hs = sorted(self.counts)
        return hs, [self.counts[h] for h in hs]


def run_reference(ns, ed, lin, pairs, planter, k, max_frequency):
    g = Graph(ns, ed, lin)
    hs, counts = planter.table()
    counts_a = np.array(counts, dtype=np.int64)
    h = np.repeat(np.array(hs, dtype=np.int64), counts_a)         # int64: the builder's ediff1d refuses uint64 here
    first = np.repeat(np.cumsum(counts_a) - counts_a, counts_a)
    refs = np.arange(len(h)) - first
    z = np.zeros(len(h), np.int64)
    index = CollisionFreeKmerIndex.from_flat_kmers(FlatKmers(h, z, refs, z.astype(float)), modulo=10007)
    for node in {n for p in pairs for n in p if len(ns[n]) >= k}:               # the stand-in hash is the package's hash
        seq = g.get_numeric_node_sequence(node)
        assert np.array_equal(ref_sv.bionumpy_hash(seq, k).astype(np.uint64), hashes_of(ns, node, k))
    out = ref_sv.sample_kmers_from_structural_variants(g, pairs, index, k, max_frequency)
    cols = {"hashes": out._hashes, "nodes": out._nodes, "ref_offsets": out._ref_offsets,
            "allele_frequencies": out._allele_frequencies}
    return hs, counts, {"dtypes": {key: str(np.asarray(c).dtype) for key, c in cols.items()},
                        **{key: [float(x) if key == "allele_frequencies" else int(x) for x in np.asarray(c)]
                           for key, c in cols.items()}}


def make_case(name, seed, k, max_frequency, bubbles, pairs=None, plant=None, density=0.5, max_count=3):
    rng = np.random.default_rng(seed)
    ns, ed, lin = bubble_graph(rng, bubbles)
    if pairs is None:
        pairs = [[3 * b + 2, 3 * b + 3] for b in range(len(bubbles))]
    pl = Planter()
    big = sorted({n for p in pairs for n in p if len(ns[n]) > k + 5})
    for node in big:                                       # background: some windows in the index, some by their
        for h in hashes_of(ns, node, k).tolist():          # reverse complement (k = 31) only
            u = rng.random()
            if u < density:
                pl.set(h, int(rng.integers(1, max_count + 1)))
            elif u < density + 0.15:
                pl.set(int(spec.revcomp(np.array([h], np.uint64), 31)[0]), int(rng.integers(1, max_count + 1)))
    if plant is not None:
        plant(ns, pl, rng)
    if not pl.counts:
        pl.set(12345, 1)                                   # the reference's index builder needs a record
    hs, counts, exp = run_reference(ns, ed, lin, [tuple(p) for p in pairs], pl, k, max_frequency)
    return {"name": name, "seed": seed, "k": k, "max_frequency": max_frequency,
            "graph": {"node_sequences": {str(n): s for n, s in ns.items()}, "edges": {str(n): e for n, e in ed.items()},
                      "linear_ref_nodes": lin},
            "pairs": [list(p) for p in pairs], "index": {"modulo": 10007, "hashes": hs, "counts": counts},
            "expected": exp}


def main():
    cases = []
    k = 31

    # sizes k+5 (skipped) and k+6 (taken) on both sides, a node whose every window is frequent (alt of bubble 3)
    def all_frequent(node):
        def plant(ns, pl, rng):
            for h in hashes_of(ns, node, 31).tolist():
                pl.set(h, 3)
        return plant
    cases.append(make_case("sizes_and_all_frequent", 1, k, 2, [(k + 5, k + 6), (k + 6, k + 5), (1, 100), (50, 300), (1, 37)],
                           plant=all_frequent(12), density=0.3))

    # the greedy rule: in the alt of bubble 0 only windows 10, 40, 41, 72, 102, 103 are valid -> 10, 41, 72, 103
    def greedy_plant(ns, pl, rng):
        hs = hashes_of(ns, 3, 31)
        assert len(set(hs.tolist())) == len(hs)
        for j, h in enumerate(hs.tolist()):
            pl.set(int(spec.revcomp(np.array([h], np.uint64), 31)[0]), 0)
            pl.set(h, 0 if j in (10, 40, 41, 72, 102, 103) else 2)
    cases.append(make_case("greedy_rule", 2, k, 2, [(1, 200), (90, 1)], plant=greedy_plant))

    # max_frequency 1, 2 and 5 over one graph with counts 1..6
    for mf in (1, 2, 5):
        cases.append(make_case("max_frequency_%d" % mf, 3, k, mf, [(1, 150), (120, 80), (60, 400)], max_count=6,
                               density=0.8))

    # k = 15: the index holds true (k = 15) reverse complements of some windows, which get_frequency never finds, and
    # k = 31 reverse complements, which it does
    def k15_plant(ns, pl, rng):
        for node in (3, 5, 6):
            for h in hashes_of(ns, node, 15).tolist():
                if rng.random() < 0.4:
                    pl.set(int(spec.revcomp(np.array([h], np.uint64), 15)[0]), 5)
    cases.append(make_case("k15_revcomp_quirk", 4, 15, 2, [(1, 120), (200, 90), (21, 20)], plant=k15_plant, density=0.2))

    # a node under two variants, ref == var, node 0 entries on either side and on both
    cases.append(make_case("shared_nodes_and_no_node", 5, k, 2, [(1, 90), (70, 110), (1, 60)],
                           pairs=[[2, 3], [0, 3], [5, 6], [6, 6], [5, 0], [0, 0], [8, 9], [5, 3]], density=0.4))

    # a node of more than 64 * 64 windows (and one over two 4096-window loads), sparse and dense validity
    cases.append(make_case("long_nodes_sparse", 6, k, 2, [(1, 4200), (9000, 64)], density=0.8))
    cases.append(make_case("long_nodes_dense", 7, k, 2, [(1, 4127 + 64), (37, 8300)], density=0.05))

    # empty input; and pairs none of whose nodes passes the size test
    cases.append(make_case("no_pairs", 8, k, 2, [(1, 100)], pairs=[]))
    cases.append(make_case("only_small_nodes", 9, k, 2, [(1, 36), (36, 2)]))
    with gzip.open(OUT, "wt") as fh:
        json.dump({"cases": cases}, fh)
    print("%s: %d cases, %d bytes" % (OUT, len(cases), os.path.getsize(OUT)))
    for c in cases:
        print("  %-28s k=%d mf=%d records=%d" % (c["name"], c["k"], c["max_frequency"], len(c["expected"]["hashes"])))


if __name__ == "__main__":
    main()
