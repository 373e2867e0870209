"""UniqueVariantKmersFinder.find_unique_kmers (dense path) at BASELINE's 3 Gbp + 5e6 SNP synthetic graph, every site a
variant (POS = 0-based site + 1, ref node = the site's ref allele, alt node = its alt allele).  Frequency index = the
variant index of bench.py's `index_build` record (the finder's records whose window crosses a node boundary).

    python tools/bench_unique_variant_kmers.py [--bases 3e9 --sites 5e6] [--verify 300]

Prints one JSON object: per-stage times (device synchronised after each), end-to-end find_unique_kmers() with the copy
back, variants/s, record counts per stage, variants of the serial pass, and with --verify the agreement of a seeded
sample of variants with the test-side restatement (tests/spec_unique_variant_kmers.py).

    python tools/bench_unique_variant_kmers.py --simple [--ab 5] [--cpu-variants 10000] [--verify 300]

times simple selection instead (find_kmers_over_variants: two per-node searches per variant, no frequency index): per-stage
and end-to-end times, and with --ab the per-node kernels (gki_forward_node_count + _emit) against the existing entry points
(gki_forward_count + _emit, no follow set, all nodes per k-mer) over the same start positions, alternating in one process;
--cpu-variants: the rate of the oracle loop (tests/spec_uvk_simple.py) on one host core over a prefix of the variants.  Every
site of this graph is a SNP whose nodes have a base: the searches start at their node, and the route of indels (a start 8
bases before the site, found on the linear reference) is not timed here."""
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


def simple(args, g, ref, alt, pos, t_graph):
    import ctypes as C
    from graph_kmer_index_amd import _lib
    from graph_kmer_index_amd.device_graph import DeviceGraph
    from graph_kmer_index_amd.unique_variant_kmers import VariantArrays, VariantToNodesArrays, _simple_selection
    lib = _lib.load()
    k, m, n = args.k, 6, len(pos)
    va = VariantArrays(pos, 1, np.arange(n), np.ones(n, np.int8))
    runs = []
    for _ in range(args.repeats + 1):                     # (the first run uploads the graph and builds the search's node records)
        t = time.perf_counter()
        d, facts = _simple_selection(g, va, ref, alt, k, m, None)
        _lib.check(lib.gki_device_synchronize())
        on_device = time.perf_counter() - t
        flat = d.to_flat_kmers()
        d.free()
        runs.append(dict(facts["timings"], on_device=on_device, end_to_end=time.perf_counter() - t))
    best = min(runs[1:], key=lambda r: r["end_to_end"])
    res = {"workload": "find_kmers_over_variants (simple selection), synthetic SNP graph %.3g bp + %d sites, k=%d, "
                       "max_variant_nodes=%d" % (args.bases, n, k, m),
           "variants": int(n), "searches": int(facts["searches"]), "output_records": int(facts["records"]),
           "stage_s": {key: round(val, 6) for key, val in best.items() if key not in ("end_to_end", "on_device")},
           "on_device_s": round(best["on_device"], 6), "end_to_end_s": round(best["end_to_end"], 6),
           "end_to_end_all_runs_s": [round(r["end_to_end"], 6) for r in runs], "variants_per_s": n / best["end_to_end"],
           "setup_s": {"graph": round(t_graph, 3)}}
    if args.ab:
        # the same start array for both: every variant's (ref node, 0) and (alt node, 0)
        h = _lib.DeviceArray.from_host
        targets = np.stack([ref, alt], 1).ravel().astype(np.int32)
        n_pos = len(targets)
        d_nodes, d_offs, d_targets = h(targets), h(np.zeros(n_pos, np.int32)), h(targets)
        d_rec = _lib.DeviceArray(n_pos + 1, np.int64)
        dg = DeviceGraph.of(g)
        n_rec = C.c_int64(0)

        def timed(fn):
            _lib.check(lib.gki_device_synchronize())
            t = time.perf_counter()
            fn()
            _lib.check(lib.gki_device_synchronize())
            return time.perf_counter() - t

        node_args = (dg.handle, k, m, d_targets.ptr, d_nodes.ptr, d_offs.ptr, n_pos, d_rec.ptr)
        all_args = (dg.handle, k, m, 0, None, d_nodes.ptr, d_offs.ptr, n_pos, d_rec.ptr)
        _lib.check(lib.gki_forward_node_count(*node_args, C.byref(n_rec)))
        n_node = n_rec.value
        _lib.check(lib.gki_forward_count(*all_args, C.byref(n_rec)))
        n_all = n_rec.value
        out_node = [_lib.DeviceArray(max(n_node, 1), dt) for dt in (np.uint64, np.uint32, np.uint64, np.float32)]
        out_all = [_lib.DeviceArray(max(n_all, 1), dt) for dt in (np.int64, np.int32, np.int16, np.int32, np.float64)]
        rounds = []
        for _ in range(args.ab + 1):                      # (first round: warm-up, dropped)
            r = {}
            r["node_count"] = timed(lambda: _lib.check(lib.gki_forward_node_count(*node_args, C.byref(n_rec))))
            r["node_emit"] = timed(lambda: _lib.check(lib.gki_forward_node_emit(*node_args, *[c.ptr for c in out_node])))
            r["all_count"] = timed(lambda: _lib.check(lib.gki_forward_count(*all_args, C.byref(n_rec))))
            r["all_emit"] = timed(lambda: _lib.check(lib.gki_forward_emit(*all_args, *[c.ptr for c in out_all])))
            rounds.append(r)
        rounds = rounds[1:]
        med = {key: float(np.median([r[key] for r in rounds])) for key in rounds[0]}
        node_s, all_s = med["node_count"] + med["node_emit"], med["all_count"] + med["all_emit"]
        res["ab"] = {"start_positions": int(n_pos), "rounds": len(rounds), "median_s": {key: round(v, 6) for key, v in med.items()},
                     "per_node_count_plus_emit_s": round(node_s, 6), "existing_count_plus_emit_s": round(all_s, 6),
                     "per_node_over_existing": round(node_s / all_s, 4), "per_node_records": int(n_node),
                     "existing_records": int(n_all),
                     "all_rounds_s": [{key: round(v, 6) for key, v in r.items()} for r in rounds]}
    if args.cpu_variants:
        import spec_uvk_simple as spec
        c = min(args.cpu_variants, n)
        t = time.perf_counter()
        exp = spec.simple_variant_kmers(g, ref, alt, pos[:c], np.arange(c), np.ones(c, np.int8), k, m)
        dt = time.perf_counter() - t
        same = all(a.dtype == b.dtype and np.array_equal(a[:len(b)], b) for a, b in
                   zip((flat._hashes, flat._nodes, flat._ref_offsets, flat._allele_frequencies), exp))
        res["cpu_oracle_loop"] = {"variants": int(c), "seconds": round(dt, 4), "variants_per_s": c / dt,
                                  "prefix_bit_exact": bool(same), "records": int(len(exp[0]))}
    if args.verify:
        import spec_uvk_simple as spec
        from graph_kmer_index_amd.unique_variant_kmers import find_kmers_over_variants
        rng = np.random.default_rng(2024)
        sample = np.sort(rng.choice(n, size=min(args.verify, n), replace=False))
        got = find_kmers_over_variants(g, VariantToNodesArrays(ref, alt),
                                       VariantArrays(pos[sample], 1, sample, np.ones(len(sample), np.int8)), k, m)
        exp = spec.simple_variant_kmers(g, ref, alt, pos[sample], sample, np.ones(len(sample), np.int8), k, m)
        same = all(a.dtype == b.dtype and np.array_equal(a, b) for a, b in
                   zip((got._hashes, got._nodes, got._ref_offsets, got._allele_frequencies), exp))
        res["verify"] = {"variants": int(len(sample)), "records": int(len(exp[0])), "bit_exact": bool(same), "seed": 2024}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=3e9)
    ap.add_argument("--sites", type=float, default=5e6)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--verify", type=int, default=0, help="number of sampled variants compared with the CPU spec")
    ap.add_argument("--modulo", type=int, default=452930477)
    ap.add_argument("--simple", action="store_true", help="time find_kmers_over_variants (simple selection) instead")
    ap.add_argument("--ab", type=int, default=0, help="--simple: rounds of per-node kernels against gki_forward_count / _emit")
    ap.add_argument("--cpu-variants", type=int, default=0, help="--simple: variants of the one-core oracle loop")
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
    if args.simple:
        print(json.dumps(simple(args, g, ref, alt, pos, t_graph)))
        return
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
