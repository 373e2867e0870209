#!/usr/bin/env python3
"""Secondary benchmark (not the headline): node counts by difference from the all-ref path and the count model on MI355X
(DESIGN.md 4.20).
  python tools/bench_haplotype_count_model.py --bases 3e9 --sites 5e6 --samples 16
The 3 Gbp + 5 M SNP graph and the variant index of tools/bench_haplotype_paths.py, and a seeded alt plane of `--samples`
diploid individuals: slot 0 takes the alt allele at about half the sites, every other slot at about 5 %.  In one run:
  base_row         HaplotypePaths.reference_node_counts: the all-ref path spelled and probed once (host clock, first call)
  slots            for slot 0 and slot 1, `--reps` repetitions after a warm-up of each route, host clock, synchronised stages:
                   whole       node_counts: spell, hash, probe (the code of the parent commit, unchanged)
                   difference  node_counts_by_difference: spell, segments, subtract, add
                   with the k-mers each route probes; the two routes' rows are asserted equal
  model            node_count_model over all `--samples` individuals by the difference route (every one of them is run; nothing
                   is scaled from a prefix), and over the first `--whole-samples` of them by both routes, asserted equal
Prints one JSON object; every section is also printed as soon as it is measured."""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from graph_kmer_index_amd import _lib, DenseKmerFinder, DeviceFlatKmers, CriticalGraphPaths
from graph_kmer_index_amd.collision_free_kmer_index import DeviceIndex
from graph_kmer_index_amd.graph import synthetic_snp_graph
from graph_kmer_index_amd.haplotype_paths import AltPlane, HaplotypePaths
from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays
from bench_haplotype_paths import IndexOnDevice, plane_row, section


def rounded(t):
    return {key: round(v, 5) if isinstance(v, float) else v for key, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=3e9)
    ap.add_argument("--sites", type=float, default=5e6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--whole-samples", type=int, default=2)
    ap.add_argument("--bins", type=int, default=5)
    ap.add_argument("--modulo", type=int, default=452930477)
    args = ap.parse_args()
    lib = _lib.load(); _lib.require_device()
    k, ploidy = 31, 2
    t0 = time.perf_counter()
    g = synthetic_snp_graph(int(args.bases), int(args.sites), k=k, seed=1234)
    alts = np.flatnonzero(g.is_ref == 0)
    v2n = VariantToNodesArrays(alts - 1, alts)
    n_lines, n_slots = len(alts), args.samples * ploidy
    result = {"bases": int(args.bases), "sites": n_lines, "nodes": g.n_nodes, "samples": args.samples, "ploidy": ploidy,
              "reps": args.reps}
    print("generated %d nodes in %.1f s" % (g.n_nodes, time.perf_counter() - t0), flush=True)
    rng = np.random.default_rng(17)
    rows = [plane_row(rng, n_lines, 0.5 if slot == 0 else 0.05) for slot in range(n_slots)]
    with _lib.DeviceScope() as s:
        plane = s.on_device(np.concatenate(rows), np.uint64)
        del rows
        cp = CriticalGraphPaths.from_graph(g, k)
        f = DenseKmerFinder(g, k, critical_graph_paths=cp, only_save_one_node_per_kmer=True, max_variant_nodes=5)
        flat = f.find_flat_on_device(); f.synchronize()
        n_int = f.interior_records()
        nb = flat.n - n_int
        bnd = DeviceFlatKmers(nb, flat.hashes.view(n_int, nb), flat.nodes.view(n_int, nb), flat.ref_offsets.view(n_int, nb),
                              flat.allele_frequencies.view(n_int, nb))
        idx = DeviceIndex.build(bnd, args.modulo)
        _lib.check(lib.gki_device_synchronize())
        flat.free()
        del bnd, flat, f
        section(result, "index", {"records": nb, "modulo": args.modulo})
        index = IndexOnDevice(idx, g.n_nodes)
        idx.probe_table()
        with HaplotypePaths(g, v2n, AltPlane(plane, n_lines, n_slots)) as paths:
            t0 = time.perf_counter()
            base = paths.reference_node_counts(index, k, g.n_nodes)
            section(result, "base_row", {"first_call_s": round(time.perf_counter() - t0, 4), "hits": int(base.sum(dtype=np.int64))})
            del base
            slots = []
            for slot in (0, 1):
                whole_t, diff_t = [], []
                whole = paths.node_counts([slot], index, k, g.n_nodes)[0]                           # warm-up
                by_difference = paths.node_counts_by_difference([slot], index, k, g.n_nodes)[0]    # warm-up
                assert np.array_equal(whole, by_difference), "slot %d: the two routes' rows differ" % slot
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    a = paths.node_counts([slot], index, k, g.n_nodes, timings=whole_t)[0]
                    whole_t[-1]["call_s"] = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    b = paths.node_counts_by_difference([slot], index, k, g.n_nodes, timings=diff_t)[0]
                    diff_t[-1]["call_s"] = time.perf_counter() - t0
                    assert np.array_equal(a, b), "slot %d: the two routes' rows differ" % slot
                med = lambda ts, key: round(statistics.median(t[key] for t in ts), 5)
                one = {"slot": slot, "taken_lines": diff_t[0]["taken_lines"], "hits": int(whole.sum(dtype=np.int64)),
                       "rows_equal": True,
                       "whole": {"kmers_probed": 2 * (whole_t[0]["letters"] - k + 1),
                                 **{key: med(whole_t, key) for key in ("spell_s", "hash_s", "probe_s", "total_s", "call_s")},
                                 "call_all_s": [round(t["call_s"], 5) for t in whole_t]},
                       "difference": {"kmers_probed": 2 * (diff_t[0]["ref_windows"] + diff_t[0]["slot_windows"]),
                                      "ref_segments": diff_t[0]["ref_segments"], "ref_windows": diff_t[0]["ref_windows"],
                                      "slot_segments": diff_t[0]["slot_segments"], "slot_windows": diff_t[0]["slot_windows"],
                                      **{key: med(diff_t, key) for key in ("spell_s", "segments_s", "subtract_s", "add_s",
                                                                          "total_s", "call_s", "segments_kernel_ms")},
                                      "call_all_s": [round(t["call_s"], 5) for t in diff_t]}}
                one["whole_over_difference_call"] = round(one["whole"]["call_s"] / one["difference"]["call_s"], 2)
                one["whole_over_difference_stages"] = round(one["whole"]["total_s"] / one["difference"]["total_s"], 2)
                print(json.dumps(one), flush=True)
                slots.append(one)
                del whole, by_difference, a, b
            section(result, "slots", slots)

            model = {}
            few = list(range(min(args.whole_samples, args.samples)))
            t0 = time.perf_counter()
            m_whole = paths.node_count_model(index, k, few, args.bins, g.n_nodes, route="whole", ploidy=ploidy)
            model["whole_route"] = {"samples": len(few), "s": round(time.perf_counter() - t0, 4)}
            t0 = time.perf_counter()
            m_few = paths.node_count_model(index, k, few, args.bins, g.n_nodes, ploidy=ploidy)
            model["difference_route_same_samples"] = {"samples": len(few), "s": round(time.perf_counter() - t0, 4)}
            assert np.array_equal(m_whole.histogram, m_few.histogram) and np.array_equal(m_whole.count_sum, m_few.count_sum)
            model["models_equal"] = True
            del m_whole, m_few
            per_slot = []
            t0 = time.perf_counter()
            m = paths.node_count_model(index, k, None, args.bins, g.n_nodes, ploidy=ploidy, timings=per_slot)
            wall = time.perf_counter() - t0
            model["difference_route_all_samples"] = {
                "samples": args.samples, "slots": len(per_slot), "s": round(wall, 4), "s_per_sample": round(wall / args.samples, 4),
                "slot_stages_s": round(sum(t["total_s"] for t in per_slot), 4),
                "kmers_probed": 2 * sum(t["ref_windows"] + t["slot_windows"] for t in per_slot),
                "individuals_in_line_0": int(m.histogram[0].sum()) // 2,
                "histogram_bytes": m.histogram.nbytes}
            section(result, "model", model)
        idx.free()
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
