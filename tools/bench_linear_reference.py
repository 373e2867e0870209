#!/usr/bin/env python3
"""Secondary benchmark (not the headline): k-mers of a linear reference, the first command of the pipeline
(`make -t 16 -s 1 -k 31 -r True -R ref.fa -n chr1 -G <size>`), on one device.
  python tools/bench_linear_reference.py --bases 2.5e8
Workload: a synthetic sequence of --bases letters (one human chromosome at the default), k = 31, spacing 1, the segment
table of `-t 16` (160 chunks, each followed by its reverse complements: 2 * bases records, inside the one-index limit).
Reported per step: the emit kernels (HIP events inside gki_linear_kmers: k_linear_emit_dense + k_linear_emit_rest) in
ms and bytes/s at 24 B per record, the 2-bit pack, the whole `make -R` from the letters in host memory to a
DeviceFlatKmers (upload, count call, allocation, pack, emit), and that flat into DeviceIndex.build.  The store ceiling
(gki_measure_store_bw: the four-column store pattern alone in a kernel) is measured in the same run on the same output
columns.  --parent-hashes N also times the only way to get these hashes on the device without this kernel, hash_reads
of a one-read batch (a single wave), at N bases, once.  Checks (size-independent): record count, and the column checksums
of nodes / allele frequencies / offsets against their closed forms.  Prints one JSON object."""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from graph_kmer_index_amd import _lib
from graph_kmer_index_amd.collision_free_kmer_index import DeviceIndex
from graph_kmer_index_amd import snp_kmer_finder as skf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=2.5e8)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modulo", type=int, default=200000033)
    ap.add_argument("--no-index", action="store_true")
    ap.add_argument("--parent-hashes", type=float, default=0, help="bases of the one-read hash_reads comparison (0: skip)")
    args = ap.parse_args()
    lib = _lib.load()
    _lib.require_device()
    n, k = int(args.bases), args.k
    rng = np.random.default_rng(1234)
    t0 = time.time()
    host = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n, dtype=np.uint8)]
    host[rng.integers(0, n, n // 1000)] = ord("N")
    t_gen = time.time() - t0
    first, count = skf.segments_of_intervals(skf.chunk_intervals(n - k, 1, args.threads), n, k, 1)
    n_rec = 2 * int(count.sum())

    whole_ms, call_ms, pack_ms, emit_ms = [], [], [], []
    dflat = None
    for step in range(args.warmup + args.steps):
        if dflat is not None:
            dflat.free()
        _lib.check(lib.gki_device_synchronize())
        t0 = time.perf_counter()
        letters = _lib.DeviceArray.from_host(host)
        t1 = time.perf_counter()
        ms = []
        dflat = skf.linear_kmers_on_device(letters, k, 1, first, count, True, kernel_ms=ms)
        t2 = time.perf_counter()
        letters.free()
        if step >= args.warmup:
            whole_ms.append((t2 - t0) * 1e3); call_ms.append((t2 - t1) * 1e3); pack_ms.append(ms[0]); emit_ms.append(ms[1])
    assert dflat.n == n_rec
    # size-independent checks of the last step's columns
    pos_sum = 2 * sum(int(c) * int(a) + int(c) * (int(c) - 1) // 2 for a, c in zip(first, count))
    checks = {"records": dflat.n,
              "nodes_all_one": dflat.nodes.checksum(dflat.n)[0] == n_rec,
              "af_all_one": dflat.allele_frequencies.checksum(dflat.n)[0] == n_rec * 0x3F800000 % 2 ** 64,
              "ref_offsets_sum": dflat.ref_offsets.checksum(dflat.n)[0] == pos_sum % 2 ** 64}
    assert all(checks.values()), checks

    index_ms = None
    if not args.no_index:
        index_ms = []
        for _ in range(2):
            _lib.check(lib.gki_device_synchronize())
            t0 = time.perf_counter()
            dev = DeviceIndex.build(dflat, args.modulo)
            _lib.check(lib.gki_device_synchronize())
            index_ms.append((time.perf_counter() - t0) * 1e3)
            dev.free()
    # the store ceiling, into the same columns, in the same run (after the index build: it overwrites them)
    bw = C.c_double(0.0)
    _lib.check(lib.gki_measure_store_bw(dflat.hashes.ptr, dflat.nodes.ptr, dflat.ref_offsets.ptr, dflat.allele_frequencies.ptr,
                                        dflat.n, C.byref(bw)))
    dflat.free()

    parent = None
    if args.parent_hashes:
        m = int(args.parent_hashes)
        reads = _lib.DeviceArray.from_host(host[:m])
        starts = _lib.DeviceArray.from_host(np.array([0, m], dtype=np.int64))
        out_start = _lib.DeviceArray(2, np.int64)
        out = _lib.DeviceArray(m, np.uint64)
        n_out = C.c_int64(0)
        _lib.check(lib.gki_device_synchronize())
        t0 = time.perf_counter()
        _lib.check(lib.gki_hash_reads(reads.ptr, starts.ptr, 1, k, 0, out_start.ptr, out.ptr, m, C.byref(n_out)))
        parent = {"bases": m, "hashes": n_out.value, "ms": (time.perf_counter() - t0) * 1e3,
                  "what": "gki_hash_reads of a one-read batch (one wave), hashes only, count + emit"}
        for a in (reads, starts, out_start, out):
            a.free()

    med = lambda v: float(np.median(v))
    emit = med(emit_ms)
    achieved = 24.0 * n_rec / (emit * 1e-3)
    print(json.dumps({
        "bench": "linear_reference", "bases": n, "k": k, "spacing": 1, "threads": args.threads, "segments": len(first),
        "records": n_rec, "steps": args.steps,
        "emit_ms": emit, "emit_ms_all": emit_ms, "emit_bytes_per_s": achieved, "bytes_per_record": 24,
        "store_ceiling_bytes_per_s": bw.value, "frac_of_ceiling": achieved / bw.value if bw.value else None,
        "pack_ms": med(pack_ms), "make_call_ms": med(call_ms), "make_with_upload_ms": med(whole_ms),
        "index_build_ms": index_ms, "index_modulo": args.modulo, "parent_hash_reads": parent,
        "generate_sequence_s": t_gen, "checks": checks}))


if __name__ == "__main__":
    main()
