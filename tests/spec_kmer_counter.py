"""Test-side restatement of the k-mer counter in NumPy: np.unique(kmers[::s], return_counts=True) (kmer_counter.py:24-43,
kmer_frequency_index.py:18-25 of the reference), a dict-backed counter with the one method the reference's consumers
call, get_frequency(kmer) -> int with no reverse complement added, and the cases recorded from the reference run with
such a counter (tests/golden/kmer_counter_reference.json.gz, written by tests/golden/make_golden_kmer_counter.py)."""
import gzip
import json
import os

import numpy as np

import spec_structural_variants as spec_sv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SV_CASES = ("sizes_and_all_frequent", "greedy_rule", "max_frequency_2", "k15_revcomp_quirk", "shared_nodes_and_no_node",
            "no_pairs")
UVK_CASES = ("snp_del_repeats_lowest", "k15_first", "shared_nodes_chunk_2", "two_chromosomes_lowest")


def unique_counts(kmers, s=1):
    """(distinct keys ascending uint64, counts int64) of kmers[::s]."""
    u, c = np.unique(np.asarray(kmers, dtype=np.uint64)[::s], return_counts=True)
    return u.astype(np.uint64), c.astype(np.int64)


class DictCounter:
    """What a consumer requires of a frequency source: get_frequency(kmer) -> int, 0 when absent."""

    def __init__(self, kmers, counts):
        self.counts = {int(k): int(c) for k, c in zip(kmers, counts)}

    def get_frequency(self, kmer):
        return self.counts.get(int(kmer), 0)


class NoReverseComplementTable(spec_sv.FrequencyTable):
    """spec_structural_variants' table with the counter's rule: the frequency of a hash is its own count alone."""

    def get_frequency(self, h, rc_k=31):
        return self.first_hit(h)


def golden():
    with gzip.open(os.path.join(ROOT, "tests", "golden", "kmer_counter_reference.json.gz"), "rt") as fh:
        return json.load(fh)


def flat_columns(e):
    """The stored FlatKmers columns of one case with their stored dtypes."""
    return tuple(np.array(e[key], dtype=np.dtype(e["dtypes"][key]))
                 for key in ("hashes", "nodes", "ref_offsets", "allele_frequencies"))


def frequency_index_inputs():
    """Key arrays for KmerFrequencyIndex.from_kmers: random, heavily repeated, one key, two extremes."""
    rng = np.random.default_rng(77)
    return {"random_62_bits": rng.integers(0, 1 << 62, size=300, dtype=np.uint64),
            "repeated": rng.integers(0, 40, size=5000, dtype=np.uint64) * np.uint64(0x0101010101010101 >> 2),
            "one_key": np.full(70, 12345, dtype=np.uint64),
            "extremes": np.array([0, (1 << 62) - 1, 0, 5, (1 << 62) - 1, 5, 5], dtype=np.uint64)}


def sv_expected_no_rc(case):
    """spec_structural_variants.sample_kmers of a stored case under the counter's rule."""
    t = NoReverseComplementTable(case["index"]["hashes"], case["index"]["counts"])
    h, n, r = spec_sv.sample_kmers(spec_sv.case_graph(case), case["pairs"], t, case["k"], case["max_frequency"])
    return h, n, r, np.ones(len(h), np.float32)


def uvk_expected_no_rc(case):
    """spec_unique_variant_kmers.unique_variant_kmers of a stored case under the counter's rule."""
    import spec_unique_variant_kmers as spec_uvk
    import uvk_golden
    g = uvk_golden.case_graph(case)
    counts = uvk_golden.case_counts(case)
    v = case["variants"]
    return spec_uvk.unique_variant_kmers(g, case["ref_nodes"], case["var_nodes"], v["positions"], v["lines"], case["k"],
                                         case["max_variant_nodes"], lambda h: counts.get(int(h), 0), case["lowest"],
                                         case["chunk_size"], chromosome_offsets=uvk_golden.chromosome_offsets(case, g))
