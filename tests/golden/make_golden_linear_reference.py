"""Generate tests/golden/linear_reference.npz by RUNNING THE REFERENCE on the cases of tests/linref_cases.py.

Run in the build container only (needs the reference checkout; tests/standins/ replace Bio and friends):

    python tests/golden/make_golden_linear_reference.py

The reference's command-line module does not import here (it needs pathos and shared_memory_wrapper), so the loop of
its `make -t N` (command_line_interface.py:105-153) is driven from this file: for every interval the reference's own
SnpKmerFinder(reference=...).find_kmers(), its get_reverse_complement_flat_kmers and from_multiple_flat_kmers when -r is
set, and np.concatenate over the chunks.  Stored: the sequences, the parameters and the reference's output columns --
data only.  The reference's `_ref_offsets` is longer than its hashes and misaligned after the first chunk; only its
LENGTH is stored (the product's column is the records' positions).
ReferenceKmerIndex.from_sequence(k = 16, 17) of one sequence goes into the same file."""
import logging
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests", "standins"), "/root/reference", ROOT, os.path.join(ROOT, "tests")]
logging.disable(logging.CRITICAL)

import numpy as np  # noqa: E402
from graph_kmer_index.snp_kmer_finder import SnpKmerFinder  # noqa: E402
from graph_kmer_index.flat_kmers import FlatKmers  # noqa: E402
from graph_kmer_index.reference_kmer_index import ReferenceKmerIndex  # noqa: E402

from linref_cases import GOLDEN, make_cases, random_sequence  # noqa: E402


def reference_make(seq, k, spacing, t, genome_size, reverse_complement):
    text = seq.tobytes().decode("ascii")
    n_jobs = t * 10
    per = (genome_size // spacing) // n_jobs
    chunks = []
    for i in range(n_jobs):
        finder = SnpKmerFinder(None, k=k, spacing=spacing, include_reverse_complements=False,
                               start_position=per * i * spacing, end_position=per * (i + 1) * spacing, reference=text)
        kmers = finder.find_kmers()
        if reverse_complement:
            kmers = FlatKmers.from_multiple_flat_kmers([kmers, kmers.get_reverse_complement_flat_kmers(k)])
        chunks.append(kmers)
    return FlatKmers(np.concatenate([c._hashes for c in chunks]), np.concatenate([c._nodes for c in chunks]),
                     np.concatenate([c._ref_offsets for c in chunks]), np.concatenate([c._allele_frequencies for c in chunks]))


def main():
    out = {}
    names = []
    for i, (name, seq, k, spacing, t, g, rc) in enumerate(make_cases()):
        flat = reference_make(seq, k, spacing, t, g, rc)
        assert flat._hashes.dtype == np.uint64 and flat._nodes.dtype == np.uint32 and flat._allele_frequencies.dtype == np.float32
        names.append(name)
        out["seq_%d" % i] = seq
        out["params_%d" % i] = np.array([k, spacing, t, g, int(rc), len(flat._ref_offsets)], dtype=np.int64)
        out["hashes_%d" % i] = flat._hashes
        out["nodes_%d" % i] = flat._nodes
        out["af_%d" % i] = flat._allele_frequencies
    out["names"] = np.array(names)
    seq = random_sequence(np.random.default_rng(77), 700)
    out["rki_seq"] = seq
    for k in (16, 17):
        idx = ReferenceKmerIndex.from_sequence(seq.tobytes().decode("ascii"), k)
        out["rki_kmers_%d" % k] = idx.kmers
        out["rki_r2i_%d" % k] = idx.ref_position_to_index
    np.savez_compressed(GOLDEN, **out)
    print("wrote %s: %d cases, %d bytes" % (GOLDEN, len(names), os.path.getsize(GOLDEN)))


if __name__ == "__main__":
    main()
