"""sample_kmers_from_structural_variants at BASELINE's 3 Gbp + 5e6 SNP synthetic graph with N inserted alt nodes (sizes
drawn uniformly from [--min-size, --max-size]; half of them random sequence, half a copy of a stretch of the reference,
whose windows over an SNP site are in the index).  Frequency index = the variant index of bench.py's `index_build`
record, as in tools/bench_unique_variant_kmers.py.

    python tools/bench_structural_variants.py [--bases 3e9 --sites 5e6 --nodes 1e5 --min-size 50 --max-size 1e4]

Prints one JSON object: windows/s of the probe pass, ms per pass (device events), end to end with the copy back, and two
baselines that are not the code under test:
  * the host route to the same answer that needs no sample_kmers_from_structural_variants: per node the windows hashed
    as 2-bit fields in NumPy, one batched CollisionFreeKmerIndex.get_frequencies over them, the greedy choice in NumPy --
    timed on the first --baseline-nodes nodes, whose records must equal the device's;
  * the device's random-request rate (gki_measure_random_loads, 2 GB table): the probe pass makes two independent random
    requests per window, so its ceiling is half that rate in windows/s."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def graph_with_inserted_nodes(g, n_new, min_size, max_size, seed):
    """g plus n_new alt nodes appended (ids g.n_nodes ...), each beside the alleles of a random site: an edge from the
    site's left segment and one to its right segment.  Returns (GraphArrays, new node ids, site ref-allele nodes)."""
    from graph_kmer_index_amd.graph import GraphArrays
    rng = np.random.default_rng([seed, 77])
    sizes = rng.integers(min_size, max_size + 1, size=n_new).astype(np.int64)
    new_start = np.concatenate([[0], np.cumsum(sizes)])
    new_seq = rng.integers(0, 4, size=int(new_start[-1]), dtype=np.uint8)
    copies = np.nonzero(rng.random(n_new) < 0.5)[0]
    src = rng.integers(0, len(g.seq) - max_size - 1, size=len(copies))
    for i, s in zip(copies.tolist(), src.tolist()):
        new_seq[new_start[i]:new_start[i + 1]] = g.seq[s:s + sizes[i]]
    alt = np.nonzero(g.is_ref == 0)[0]
    site = np.sort(rng.choice(len(alt), size=n_new, replace=len(alt) < n_new))
    ref_allele = alt[site] - 1
    pred = g.rev_edges[g.rev_start[ref_allele]].astype(np.int64)          # the segment's last chunk
    succ = g.edges[g.edge_start[ref_allele]]
    new_ids = g.n_nodes + np.arange(n_new)
    edges = np.insert(g.edges, g.edge_start[pred + 1], new_ids.astype(np.int32))
    deg = np.diff(g.edge_start)
    np.add.at(deg, pred, 1)
    edge_start = np.concatenate([[0], np.cumsum(np.concatenate([deg, np.ones(n_new, np.int64)]))])
    edges = np.concatenate([edges, succ])
    g2 = GraphArrays(np.concatenate([g.node_size, sizes.astype(np.int32)]), np.concatenate([g.seq, new_seq]), edge_start,
                     edges, np.concatenate([g.is_ref, np.zeros(n_new, np.uint8)]),
                     np.concatenate([g.allele_freq, np.full(n_new, 0.01)]), first_node=0, chromosome_start_nodes=[0],
                     node_to_ref_offset=np.concatenate([g.node_to_ref_offset, np.zeros(n_new, np.int64)]))
    return g2, new_ids, ref_allele


def host_route(g, nodes, index, k, max_frequency):
    """The same records without the new entry points: NumPy hashing, batched get_frequencies, NumPy greedy."""
    shifts = (2 * np.arange(k)).astype(np.uint64)
    hashes, counts = [], []
    for n in nodes.tolist():
        codes = g.get_numeric_node_sequence(n).astype(np.uint64)
        if len(codes) > k + 5:
            w = np.lib.stride_tricks.sliding_window_view(codes, k)
            hashes.append((w << shifts[None, :]).sum(axis=1, dtype=np.uint64))
            counts.append((n, len(hashes[-1])))
    if not hashes:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint32), 0
    allh = np.concatenate(hashes)
    f = index.get_frequencies(allh)
    out_h, out_n, at = [], [], 0
    for n, c in counts:
        valid = np.nonzero(f[at:at + c] < max_frequency)[0]
        chosen, prev = [], -10000
        while True:
            i = int(np.searchsorted(valid, prev + k))
            if i == len(valid):
                break
            prev = int(valid[i])
            chosen.append(prev)
        out_h.append(allh[at:at + c][chosen])
        out_n.append(np.full(len(chosen), n, np.uint32))
        at += c
    return np.concatenate(out_h), np.concatenate(out_n), len(allh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=3e9)
    ap.add_argument("--sites", type=float, default=5e6)
    ap.add_argument("--nodes", type=float, default=1e5)
    ap.add_argument("--min-size", type=float, default=50)
    ap.add_argument("--max-size", type=float, default=1e4)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--max-frequency", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-nodes", type=int, default=2000)
    ap.add_argument("--modulo", type=int, default=452930477)
    args = ap.parse_args()
    import ctypes as C
    from graph_kmer_index_amd import _lib, DenseKmerFinder, CollisionFreeKmerIndex
    from graph_kmer_index_amd import structural_variants as sv
    from graph_kmer_index_amd.collision_free_kmer_index import DeviceIndex
    from graph_kmer_index_amd.flat_kmers import DeviceFlatKmers
    from graph_kmer_index_amd.graph import synthetic_snp_graph
    from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays
    lib = _lib.load()
    _lib.require_device()
    k = args.k
    t = time.perf_counter()
    g = synthetic_snp_graph(int(args.bases), int(args.sites), k=k, seed=1234)
    t_graph = time.perf_counter() - t
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
    if g._device is not None:
        g._device.close()
        g._device = None
    t_index = time.perf_counter() - t
    index = CollisionFreeKmerIndex(_modulo=args.modulo)
    index._device = dev
    index._frequencies = dev.frequencies.to_host(nb)          # the host route's get_frequencies gathers from it
    t = time.perf_counter()
    g2, new_ids, ref_allele = graph_with_inserted_nodes(g, int(args.nodes), int(args.min_size), int(args.max_size), 1234)
    t_insert = time.perf_counter() - t
    v2n = VariantToNodesArrays(ref_allele, new_ids)
    runs = []
    for _ in range(args.repeats):
        flat = sv.sample_kmers_from_structural_variants(g2, v2n, index, k, args.max_frequency)
        runs.append(dict(sv.last_timings))
    best = min(runs, key=lambda r: r["end_to_end"])
    counts = dict(sv.last_counts)
    windows = counts["windows"]
    probe_ms = min(r["kernel_ms"]["probe"] for r in runs)
    rate = C.c_double(0.0)
    _lib.check(lib.gki_measure_random_loads(2 << 30, 1 << 31, C.byref(rate)))
    windows_per_s = windows / (probe_ms * 1e-3)
    # the host route on the first nodes, and its agreement with the device's records for them
    sub = new_ids[:args.baseline_nodes]
    t = time.perf_counter()
    bh, bn, b_windows = host_route(g2, sub, index, k, args.max_frequency)
    t_host = time.perf_counter() - t
    sel = np.isin(flat._nodes, sub.astype(np.uint32))
    same = bool(np.array_equal(flat._hashes[sel], bh) and np.array_equal(flat._nodes[sel], bn))
    res = {"workload": "sample_kmers_from_structural_variants, synthetic SNP graph %.3g bp + %d sites + %d inserted alt nodes "
                       "of %d..%d bases (half random, half copies of reference stretches), k=%d, max_frequency=%d"
                       % (args.bases, int(args.sites), len(new_ids), int(args.min_size), int(args.max_size), k,
                          args.max_frequency),
           "counts": counts, "index_records": int(nb), "modulo": args.modulo,
           "kernel_ms": {key: round(min(r["kernel_ms"][key] for r in runs), 4) for key in best["kernel_ms"]},
           "probe_windows_per_s": windows_per_s,
           "stage_s": {key: round(val, 6) for key, val in best.items() if key not in ("end_to_end", "kernel_ms")},
           "end_to_end_s": round(best["end_to_end"], 6), "end_to_end_all_runs_s": [round(r["end_to_end"], 6) for r in runs],
           "end_to_end_windows_per_s": windows / best["end_to_end"],
           "random_requests_per_s": rate.value, "probe_ceiling_windows_per_s": rate.value / 2,
           "probe_fraction_of_ceiling": windows_per_s / (rate.value / 2),
           "host_route": {"nodes": int(len(sub)), "windows": int(b_windows), "s": round(t_host, 4),
                          "windows_per_s": b_windows / t_host if t_host else None, "records_equal_device": same,
                          "scaled_to_all_windows_s": t_host * windows / b_windows if b_windows else None},
           "output_records": int(len(flat._hashes)),
           "setup_s": {"graph": round(t_graph, 3), "variant_index": round(t_index, 3), "insert_nodes": round(t_insert, 3)}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
