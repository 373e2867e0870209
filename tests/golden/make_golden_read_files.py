"""Generate tests/golden/read_files_reference.json.gz by RUNNING THE REFERENCE's ReadKmers.from_fasta_file on the FASTA
files of tests/read_file_cases.py GOLDEN_CASES.

Run in the build container only (needs /root/reference; tests/standins/ replace Bio and friends):

    python tests/golden/make_golden_read_files.py

Stored, per case and per k of read_file_cases.GOLDEN_KS: for every read the hashes the reference yields for it, the
forward pass first and the reverse-complement pass second (read_kmers.py:21-26 chains the two).  A read shorter than k is
stored as null: the reference's answer for it is not defined (np.convolve(..., 'valid') swaps its arguments when the
read is the shorter one and returns k - len + 1 numbers that are no k-mer hashes).  Data only.
"""
import gzip
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests", "standins"), "/root/reference", ROOT, os.path.join(ROOT, "tests"), HERE]

import numpy as np  # noqa: E402

from graph_kmer_index.read_kmers import ReadKmers  # noqa: E402

import read_file_cases as cases  # noqa: E402
import spec_read_files as spec  # noqa: E402

OUT = os.path.join(HERE, "read_files_reference.json.gz")


def reference_hashes(data, k):
    """{"forward": [...], "reverse": [...]}: per read the list of hashes the reference yields, or None for a read
    shorter than k."""
    reads, _, _ = spec.parse(data, "fasta")
    with tempfile.TemporaryDirectory(prefix="gki_read_files_") as tmp:
        path = os.path.join(tmp, "reads.fa")
        with open(path, "wb") as fh:
            fh.write(data)
        per_read = [np.asarray(x) for x in ReadKmers.from_fasta_file(path, k)]
    assert len(per_read) == 2 * len(reads), (len(per_read), len(reads))

    def column(arrays):
        return [[int(np.uint64(h)) for h in a] if len(r) >= k else None for a, r in zip(arrays, reads)]
    return {"forward": column(per_read[:len(reads)]), "reverse": column(per_read[len(reads):])}


def run_all():
    return {name: {str(k): reference_hashes(data, k) for k in cases.GOLDEN_KS} for name, data in cases.GOLDEN_CASES.items()}


def main():
    out = run_all()
    with gzip.GzipFile(OUT, "wb", mtime=0) as fh:
        fh.write(json.dumps(out).encode("ascii"))
    print("%s: %d bytes" % (OUT, os.path.getsize(OUT)))
    for name, by_k in out.items():
        print("  %-24s %s" % (name, "  ".join("k=%s: %d reads, %d undefined" % (k, len(e["forward"]), sum(x is None for x in e["forward"]))
                                              for k, e in by_k.items())))


if __name__ == "__main__":
    main()
