"""UniqueVariantKmersFinder.find_unique_kmers (dense path) at BASELINE's 3 Gbp + 5e6 SNP synthetic graph, every site a
variant (POS = 0-based site + 1, ref node = the site's ref allele, alt node = its alt allele).  Frequency index = the
variant index of bench.py's `index_build` record (the finder's records whose window crosses a node boundary).

    python tools/bench_unique_variant_kmers.py [--bases 3e9 --sites 5e6] [--verify 300]

Prints one JSON object: per-stage times (device synchronised after each), end-to-end find_unique_kmers() with the copy
back, variants/s, record counts per stage, variants of the serial pass, and with --verify the agreement of a seeded
sample of variants with the test-side restatement (tests/spec_unique_variant_kmers.py)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


class PositionIdOfGraph:
    def __init__(self, base):
        self._base = base

    def get(self, nodes, offsets):
        return self._base[np.asarray(nodes, dtype=np.int64)] + np.asarray(offsets, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=3e9)
    ap.add_argument("--sites", type=float, default=5e6)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--verify", type=int, default=0, help="number of sampled variants compared with the CPU spec")
    ap.add_argument("--modulo", type=int, default=452930477)
    args = ap.parse_args()
    from graph_kmer_index_amd import _lib, DenseKmerFinder, CollisionFreeKmerIndex
    from graph_kmer_index_amd.collision_free_kmer_index import DeviceIndex
    from graph_kmer_index_amd.flat_kmers import DeviceFlatKmers
    from graph_kmer_index_amd.graph import synthetic_snp_graph
    from graph_kmer_index_amd.unique_variant_kmers import UniqueVariantKmersFinder, VariantArrays, VariantToNodesArrays
    lib = _lib.load()
    _lib.require_device()
    k = args.k
    t = time.perf_counter()
    g = synthetic_snp_graph(int(args.bases), int(args.sites), k=k, seed=1234)
    t_graph = time.perf_counter() - t
    alt = np.nonzero(g.is_ref == 0)[0]
    ref = alt - 1
    pos = np.asarray(g.node_to_ref_offset)[ref] + 1
    keep = pos - 2 - 4 * (len(range(2, k - 2)[::4]) - 1) >= 0
    ref, alt, pos = ref[keep], alt[keep], pos[keep]
    # the variant index: boundary records of the whole-graph finder (bench.py secondary_records)
    t = time.perf_counter()
    finder = DenseKmerFinder(g, k, max_variant_nodes=4)
    out = finder.find_flat_on_device()
    n_int = finder.interior_records()
    nb = out.n - n_int
    bnd = DeviceFlatKmers(nb, out.hashes.view(n_int, nb), out.nodes.view(n_int, nb), out.ref_offsets.view(n_int, nb),
                          out.allele_frequencies.view(n_int, nb))
    dev = DeviceIndex.build(bnd, args.modulo)
    _lib.check(lib.gki_device_synchronize())
    out.free()
    finder.close()
    t_index = time.perf_counter() - t
    index = CollisionFreeKmerIndex(_modulo=args.modulo)
    index._device = dev
    pid = PositionIdOfGraph(g.position_id_base())
    v2n = VariantToNodesArrays(ref, alt)
    variants = VariantArrays(pos, 1, np.arange(len(pos)))
    uvk = UniqueVariantKmersFinder(g, v2n, variants, k, 6, kmer_index_with_frequencies=index, use_dense_kmer_finder=True,
                                   position_id_index=pid)
    runs = []
    for _ in range(args.repeats):
        flat = uvk.find_unique_kmers()
        runs.append(dict(uvk.last_timings))
    best = min(runs, key=lambda r: r["end_to_end"])
    res = {"workload": "UniqueVariantKmersFinder dense path, synthetic SNP graph %.3g bp + %d sites, k=%d, max_variant_nodes=6"
                       % (args.bases, len(pos), k),
           "variants": int(len(pos)), "index_records": int(nb), "modulo": args.modulo,
           "stage_s": {key: round(val, 6) for key, val in best.items() if key != "end_to_end"},
           "end_to_end_s": round(best["end_to_end"], 6), "end_to_end_all_runs_s": [round(r["end_to_end"], 6) for r in runs],
           "variants_per_s": len(pos) / best["end_to_end"], "counts": uvk.last_counts,
           "serial_pass_variants": uvk.last_serial_variants, "output_records": int(len(flat._hashes)),
           "setup_s": {"graph": round(t_graph, 3), "variant_index": round(t_index, 3)}}
    if args.verify:
        import spec_unique_variant_kmers as spec
        from graph_kmer_index_amd.kmer_hashing import kmer_hash_to_reverse_complement_hash
        fr = dev.frequencies

        def first(q):
            n, p = dev.get_small([q], max_hits=2 ** 62, capacity=1)[0]
            return int(fr.view(int(p[0]), 1).to_host()[0]) if n else 0

        def frequency(h):
            return first(h) + first(int(kmer_hash_to_reverse_complement_hash(h, 31)))

        rng = np.random.default_rng(2024)
        sample = np.sort(rng.choice(len(pos), size=min(args.verify, len(pos)), replace=False))
        sub = UniqueVariantKmersFinder(g, v2n, VariantArrays(pos[sample], 1, sample), k, 6,
                                       kmer_index_with_frequencies=index, use_dense_kmer_finder=True, position_id_index=pid)
        got = sub.find_unique_kmers()
        exp = spec.unique_variant_kmers(g, ref, alt, pos[sample], sample, k, 6, frequency)
        same = all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in
                   zip((got._hashes, got._nodes, got._ref_offsets, got._allele_frequencies), exp))
        res["verify"] = {"variants": int(len(sample)), "records": int(len(exp[0])), "bit_exact": bool(same), "seed": 2024}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
