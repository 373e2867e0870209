#!/usr/bin/env python3
"""Secondary benchmark (not the headline): haplotype paths on MI355X.
  python tools/bench_haplotype_paths.py --bases 3e9 --sites 5e6
The 3 Gbp + 5 M SNP graph of the other tools (synthetic_snp_graph) and a seeded alt plane of two slots: slot 0 takes the alt
allele at about half the sites, slot 1 at about 5 %.  In one run:
  spell            per slot k_hap_spell's device time and the device time of a device-to-device copy of the same n_out
                   bytes, the two alternated, `--reps` repetitions after a warm-up, medians, both by device events; the count
                   pass (drops, scan, cuts, tile search) by device events in the same calls
  alt_nodes        gki_haplotype_alt_nodes_count / _emit for `--all-slots` slots (rows of about 5 % alt), device events and the
                   host clock around both calls, the nodes left on the device
  host_spelling_s  the NumPy mask compaction of graph.synthetic_haplotype_sequence on the same graph, a SINGLE run
  node_counts      per slot the split spell / hash / probe and the whole call (host clock, synchronised), the variant index
                   built as in tools/bench_index.py from the records tools/bench_reads.py indexes (those whose window
                   touches a variant node: all records of the 3 Gbp graph do not fit one index's int32 directory)
Prints one JSON object; every section is also printed as soon as it is measured."""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from graph_kmer_index_amd import _lib, DenseKmerFinder, DeviceFlatKmers, CriticalGraphPaths
from graph_kmer_index_amd.collision_free_kmer_index import DeviceIndex
from graph_kmer_index_amd.graph import synthetic_snp_graph, synthetic_haplotype_sequence
from graph_kmer_index_amd.haplotype_paths import AltPlane, HaplotypePaths
from graph_kmer_index_amd.unique_variant_kmers import VariantToNodesArrays


def plane_row(rng, n_lines, p_alt):
    """uint64[ceil(n_lines / 64)]: bit v % 64 of word v // 64 set with probability p_alt."""
    bits = np.zeros(((n_lines + 63) // 64) * 64, dtype=np.uint8)
    bits[:n_lines] = rng.random(n_lines) < p_alt
    return np.packbits(bits, bitorder="little").view(np.uint64)


class IndexOnDevice:
    """What node_counts asks of a CollisionFreeKmerIndex, for an index that was built and stays on the device."""

    def __init__(self, device_index, n_nodes):
        self._device, self._n_nodes = device_index, n_nodes

    def _device_index(self):
        return self._device

    def max_node_id(self):
        return self._n_nodes - 1


def section(result, name, value):
    result[name] = value
    print(json.dumps({name: value}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=3e9)
    ap.add_argument("--sites", type=float, default=5e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--all-slots", type=int, default=5008)
    ap.add_argument("--modulo", type=int, default=452930477)
    ap.add_argument("--skip-node-counts", action="store_true")
    args = ap.parse_args()
    lib = _lib.load(); _lib.require_device()
    k = 31
    t0 = time.perf_counter()
    g = synthetic_snp_graph(int(args.bases), int(args.sites), k=k, seed=1234)
    alts = np.flatnonzero(g.is_ref == 0)
    v2n = VariantToNodesArrays(alts - 1, alts)
    n_lines, words = len(alts), (len(alts) + 63) // 64
    result = {"bases": int(args.bases), "sites": n_lines, "nodes": g.n_nodes, "seq_bytes": len(g.seq), "reps": args.reps}
    print("generated %d nodes in %.1f s" % (g.n_nodes, time.perf_counter() - t0), flush=True)
    rng = np.random.default_rng(17)
    rows = [plane_row(rng, n_lines, 0.5), plane_row(rng, n_lines, 0.05)]
    with _lib.DeviceScope() as s:
        plane = s.on_device(np.concatenate(rows), np.uint64)
        t0 = time.perf_counter()
        paths = HaplotypePaths(g, v2n, AltPlane(plane, n_lines, 2))
        section(result, "plan_create_s", round(time.perf_counter() - t0, 3))
        with paths:
            spell = {}
            scratch = s.array(len(g.seq), np.uint8)
            for slot, name in ((0, "half_alt"), (1, "five_percent_alt")):
                paths.sequence(slot).free()                                     # warm-up
                spell_ms, copy_ms, count_ms, n_out = [], [], [], 0
                for _ in range(args.reps):
                    with _lib.DeviceScope() as r:
                        ref = r.keep(paths.sequence(slot))
                        n_out = ref.letters.n
                        spell_ms.append(ref.timings["spell_kernel_ms"]); count_ms.append(ref.timings["count_kernel_ms"])
                        ms = C.c_float(0)
                        _lib.check(lib.gki_measure_copy_ms(scratch.ptr, ref.letters.ptr, n_out, C.byref(ms)))
                        copy_ms.append(float(ms.value))
                med = statistics.median
                spell[name] = {"n_out": n_out, "alt_taken": round(int(np.unpackbits(rows[slot].view(np.uint8)).sum()) / max(n_lines, 1), 4),
                               "k_hap_spell_ms": round(med(spell_ms), 4), "k_hap_spell_all_ms": [round(x, 4) for x in spell_ms],
                               "device_copy_of_n_out_bytes_ms": round(med(copy_ms), 4),
                               "device_copy_all_ms": [round(x, 4) for x in copy_ms],
                               "spell_over_copy": round(med(spell_ms) / med(copy_ms), 3),
                               "spell_GBps_read_plus_written": round(2 * n_out / med(spell_ms) / 1e6, 1),
                               "count_pass_ms": round(med(count_ms), 4), "count_pass_all_ms": [round(x, 4) for x in count_ms]}
            scratch.free()
            section(result, "spell", spell)

            # the alt nodes of many slots: rows of about 5 % alt, 16 of them drawn and repeated
            h = args.all_slots
            drawn = np.stack([plane_row(rng, n_lines, 0.05) for _ in range(min(16, h))])
            with _lib.DeviceScope() as a:
                many = a.array(max(h * words, 1), np.uint64)
                block = a.on_device(drawn.reshape(-1), np.uint64)
                for first in range(0, h, len(drawn)):
                    n = min(len(drawn), h - first)
                    _lib.check(lib.gki_memcpy_d2d(C.c_void_p(many.ptr.value + first * words * 8), block.ptr, n * words * 8))
                start = a.array(h + 1, np.int64)
                runs = []
                for _ in range(2):                                              # the second run is reported
                    n_nodes, ms_count, ms_emit = C.c_int64(0), C.c_float(0), C.c_float(0)
                    _lib.check(lib.gki_device_synchronize())
                    t0 = time.perf_counter()
                    _lib.check(lib.gki_haplotype_alt_nodes_count(paths._plan, many.ptr, h, start.ptr, C.byref(n_nodes), C.byref(ms_count)))
                    with _lib.DeviceScope() as o:
                        nodes = o.array(max(n_nodes.value, 1), np.uint32)
                        _lib.check(lib.gki_haplotype_alt_nodes_emit(paths._plan, many.ptr, h, nodes.ptr, C.byref(ms_emit)))
                        _lib.check(lib.gki_device_synchronize())
                        wall = time.perf_counter() - t0
                    runs.append({"slots": h, "plane_bytes": h * words * 8, "alt_nodes": n_nodes.value,
                                 "count_kernels_ms": round(float(ms_count.value), 3), "emit_kernel_ms": round(float(ms_emit.value), 3),
                                 "both_calls_s": round(wall, 4)})
                section(result, "alt_nodes", runs[-1])

            t0 = time.perf_counter()
            host = synthetic_haplotype_sequence(g)
            section(result, "host_spelling_s", round(time.perf_counter() - t0, 3))
            result["host_spelling_letters"] = len(host)
            del host
            section(result, "host_spelling_over_device_spell_plus_count",
                    round(result["host_spelling_s"] * 1e3 / (spell["half_alt"]["k_hap_spell_ms"] + spell["half_alt"]["count_pass_ms"]), 1))

            if not args.skip_node_counts:
                try:
                    cp = CriticalGraphPaths.from_graph(g, k)
                    f = DenseKmerFinder(g, k, critical_graph_paths=cp, only_save_one_node_per_kmer=True, max_variant_nodes=5)
                    flat = f.find_flat_on_device(); f.synchronize()
                    # the variant index of tools/bench_reads.py: the records whose window touches a variant node, which the
                    # finder emits behind the interior ones
                    n_int = f.interior_records()
                    nb = flat.n - n_int
                    bnd = DeviceFlatKmers(nb, flat.hashes.view(n_int, nb), flat.nodes.view(n_int, nb),
                                          flat.ref_offsets.view(n_int, nb), flat.allele_frequencies.view(n_int, nb))
                    print("found %d records, %d of them for the variant index" % (flat.n, nb), flush=True)
                    t0 = time.perf_counter()
                    idx = DeviceIndex.build(bnd, args.modulo)
                    _lib.check(lib.gki_device_synchronize())
                    section(result, "index", {"records": nb, "modulo": args.modulo, "build_s": round(time.perf_counter() - t0, 3)})
                    flat.free()
                    del bnd, flat, f
                    index = IndexOnDevice(idx, g.n_nodes)
                    idx.probe_table()
                    timings = []
                    paths.node_counts([1], index, k, g.n_nodes)                 # warm-up
                    print("node counts: warm-up done", flush=True)
                    for slot in (0, 1):
                        row = paths.node_counts([slot], index, k, g.n_nodes, timings=timings)[0]
                        t = timings[-1]
                        t.update({key: round(v, 4) for key, v in t.items() if isinstance(v, float)})
                        t["kmers_probed"] = 2 * (t["letters"] - k + 1)
                        t["hits"] = int(row.sum(dtype=np.int64))
                        print(json.dumps(t), flush=True)
                    section(result, "node_counts", timings)
                    idx.free()
                except (_lib.GkiError, MemoryError) as e:
                    section(result, "node_counts", {"not_measured": str(e)})
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
