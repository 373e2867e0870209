"""Generate tests/golden/kmer_counter_reference.json.gz by RUNNING THE REFERENCE with a k-mer counter as frequency source.

Run in the build container only (needs /root/reference; tests/standins/ replace obgraph and friends):

    python tests/golden/make_golden_kmer_counter.py

The reference's KmerCounter stores its counts in an `npstructures` table, which is not available; what its consumers call
is get_frequency(kmer) alone, so they are run live with a dict-backed counter (tests/spec_kmer_counter.py DictCounter)
over the (hash, count) pairs the stored cases of sv_kmers_reference.json.gz / uvk_reference.json.gz already hold:
  * sample_kmers_from_structural_variants on spec_kmer_counter.SV_CASES,
  * UniqueVariantKmersFinder (dense path, one finder per chunk) on spec_kmer_counter.UVK_CASES,
  * KmerFrequencyIndex.from_kmers on spec_kmer_counter.frequency_index_inputs(), and KmerFrequencyIndex.get on probes of
    those arrays (a value, or "IndexError" where the reference indexes past its array).
Stored: output columns with their dtypes -- data only.
"""
import gzip
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests", "standins"), "/root/reference", ROOT, os.path.join(ROOT, "tests"), HERE]

import numpy as np  # noqa: E402

import make_golden_sv_kmers as sv_driver  # noqa: E402  (stands bionumpy_hash in, as for sv_kmers_reference.json.gz)
import make_golden_uvk as uvk_driver  # noqa: E402
from obgraph import Graph  # noqa: E402
from obgraph.position_id import PositionId  # noqa: E402
from graph_kmer_index.flat_kmers import FlatKmers  # noqa: E402
from graph_kmer_index.kmer_frequency_index import KmerFrequencyIndex  # noqa: E402
from graph_kmer_index.unique_variant_kmers import UniqueVariantKmersFinder  # noqa: E402

import spec_kmer_counter as spec  # noqa: E402
import spec_structural_variants as spec_sv  # noqa: E402
import uvk_golden  # noqa: E402

OUT = os.path.join(HERE, "kmer_counter_reference.json.gz")


def columns(flat):
    cols = {"hashes": flat._hashes, "nodes": flat._nodes, "ref_offsets": flat._ref_offsets,
            "allele_frequencies": flat._allele_frequencies}
    return {"dtypes": {key: str(np.asarray(c).dtype) for key, c in cols.items()},
            **{key: [float(x) if key == "allele_frequencies" else int(x) for x in np.asarray(c)] for key, c in cols.items()}}


def reference_sv(case):
    gr = case["graph"]
    g = Graph({int(n): s for n, s in gr["node_sequences"].items()}, {int(n): e for n, e in gr["edges"].items()},
              gr["linear_ref_nodes"])
    counter = spec.DictCounter(case["index"]["hashes"], case["index"]["counts"])
    return sv_driver.ref_sv.sample_kmers_from_structural_variants(g, [tuple(p) for p in case["pairs"]], counter, case["k"],
                                                                  case["max_frequency"])


def reference_uvk(case):
    gr = case["graph"]
    g = uvk_driver.PositionalGraph({int(n): s for n, s in gr["node_sequences"].items()},
                                   {int(n): e for n, e in gr["edges"].items()}, gr["linear_ref_nodes"],
                                   chromosome_start_nodes=gr["chromosome_start_nodes"])
    pid = PositionId.from_graph(g)
    counter = spec.DictCounter(case["index"]["hashes"], case["index"]["counts"])
    v = case["variants"]
    vs = [uvk_driver._Variant(p, c, i) for p, c, i in zip(v["positions"], v["chromosomes"], v["lines"])]
    cs = case["chunk_size"]
    chunks = [vs] if cs is None else [vs[i:i + cs] for i in range(0, len(vs), cs)]
    flats = []
    for chunk in chunks:
        u = UniqueVariantKmersFinder(g, uvk_driver._V2N(case["ref_nodes"], case["var_nodes"]), chunk, case["k"],
                                     case["max_variant_nodes"], kmer_index_with_frequencies=counter,
                                     do_not_choose_lowest_frequency_kmers=not case["lowest"], use_dense_kmer_finder=True,
                                     position_id_index=pid)
        flats.append(u.find_unique_kmers())
    return FlatKmers.from_multiple_flat_kmers(flats)


def reference_frequency_index(kmers):
    idx = KmerFrequencyIndex.from_kmers(kmers)
    probes = sorted({int(x) for x in idx._kmers[:3]} | {int(x) for x in idx._kmers[-2:]} | {int(idx._kmers[0]) + 1, 1 << 63})
    got = []
    for q in probes:
        try:
            got.append(int(idx.get(np.uint64(q))))
        except IndexError:
            got.append("IndexError")
    return {"kmers": [int(x) for x in idx._kmers], "frequencies": [int(x) for x in idx._frequencies],
            "dtypes": {"kmers": str(idx._kmers.dtype), "frequencies": str(idx._frequencies.dtype)},
            "probes": probes, "get": got}


def main():
    sv = {c["name"]: c for c in spec_sv.load_cases()}
    uvk = {c["name"]: c for c in uvk_golden.load_cases()}
    out = {"sv": {name: columns(reference_sv(sv[name])) for name in spec.SV_CASES},
           "uvk": {name: columns(reference_uvk(uvk[name])) for name in spec.UVK_CASES},
           "frequency_index": {name: reference_frequency_index(k) for name, k in spec.frequency_index_inputs().items()}}
    with gzip.open(OUT, "wt") as fh:
        json.dump(out, fh)
    print("%s: %d bytes" % (OUT, os.path.getsize(OUT)))
    for key in ("sv", "uvk"):
        for name, e in out[key].items():
            print("  %-4s %-28s records=%d" % (key, name, len(e["hashes"])))


if __name__ == "__main__":
    main()
