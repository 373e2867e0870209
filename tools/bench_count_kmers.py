#!/usr/bin/env python3
"""Secondary benchmark (not the headline): unique k-mers with counts of one chromosome's linear-reference k-mers, and
lookups in the counter over them (`count_kmers` of the pipeline), on one device.
  python tools/bench_count_kmers.py --bases 2.5e8
Workload: the k-mers tools/bench_linear_reference.py makes (a synthetic sequence of --bases letters, k = 31, spacing 1,
the segment table of `-t 16`, each chunk followed by its reverse complements: 2 * bases = 5e8 keys at the default), left
in HBM.  Every GPU step is a child process of this tool under its own `timeout -k 10`; the tool stops at the first step
that fails.  Steps:
  count   gki_unique_counts_count + gki_unique_counts_emit on the hashes column (key_bits = 2k): keys/s, and the bytes
          the passes move per key by the model of DESIGN.md 4.10 against the 8 TB/s peak; the store ceiling of the same
          run (gki_measure_store_bw); np.unique(return_counts=True) on the host for a 1e7-key prefix, which must equal
          the device's answer for that prefix
  lookup  a KmerCounter's device counter over the same unique keys: lookups/s for present and for absent queries, beside
          gki_measure_random_loads from the same run
Prints one JSON object (and writes it to --out when given)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES_PER_S = 8.0e12


def reference_kmers(bases, k, threads):
    """(DeviceFlatKmers of the linear-reference k-mers, seconds to generate the letters on the host)."""
    import numpy as np
    from graph_kmer_index_amd import _lib
    from graph_kmer_index_amd import snp_kmer_finder as skf
    rng = np.random.default_rng(1234)
    t0 = time.time()
    host = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, bases, dtype=np.uint8)]
    t_gen = time.time() - t0
    first, count = skf.segments_of_intervals(skf.chunk_intervals(bases - k, 1, threads), bases, k, 1)
    letters = _lib.DeviceArray.from_host(host)
    dflat = skf.linear_kmers_on_device(letters, k, 1, first, count, True)
    letters.free()
    return dflat, t_gen


def model_bytes_per_key(key_bits):
    """Per pass: 8 B histogram read + 8 B scatter read + 8 B scatter write; run heads: 8 B count read + 8 B emit read;
    per unique key 8 + 8 B written and 8 + 8 + 8 B for the run lengths (counted per key: an upper bound)."""
    passes = (key_bits + 7) // 8
    return passes * 24 + 16 + 40


def step_count(args):
    import numpy as np
    from graph_kmer_index_amd import _lib
    from graph_kmer_index_amd.kmer_counter import unique_counts_on_device
    lib = _lib.load()
    _lib.require_device()
    k, key_bits = args.k, 2 * args.k
    dflat, t_gen = reference_kmers(int(args.bases), k, args.threads)
    n = dflat.n
    keys = dflat.hashes.view(0, n)
    runs, n_unique = [], None
    for step in range(args.warmup + args.steps):
        _lib.check(lib.gki_device_synchronize())
        t0 = time.perf_counter()
        u, c = unique_counts_on_device(keys, 1, key_bits)
        _lib.check(lib.gki_device_synchronize())
        wall = (time.perf_counter() - t0) * 1e3
        ms = dict(unique_counts_on_device.last_kernel_ms)
        if step >= args.warmup:
            runs.append(dict(ms, wall_ms=wall, kernel_ms=ms["sort"] + ms["run_heads"] + ms["emit"]))
        n_unique = u.n
        total = c.checksum()[0]
        assert total == n, (total, n)                   # the counts add up to the number of keys
        if step < args.warmup + args.steps - 1:
            u.free(); c.free()
    # the host's np.unique on a prefix, and the device's answer for the same prefix
    m = min(n, int(args.host_prefix))
    prefix = dflat.hashes.view(0, m)
    host_keys = prefix.to_host()
    t0 = time.perf_counter()
    hu, hc = np.unique(host_keys, return_counts=True)
    host_s = time.perf_counter() - t0
    du, dc = unique_counts_on_device(prefix, 1, key_bits)
    prefix_equal = bool(np.array_equal(du.to_host(), hu) and np.array_equal(dc.to_host(), hc))
    du.free(); dc.free()
    u.free(); c.free()
    assert prefix_equal
    bw = C.c_double(0.0)
    _lib.check(lib.gki_measure_store_bw(dflat.hashes.ptr, dflat.nodes.ptr, dflat.ref_offsets.ptr, dflat.allele_frequencies.ptr,
                                        n, C.byref(bw)))
    dflat.free()
    best = min(runs, key=lambda r: r["kernel_ms"])
    bpk = model_bytes_per_key(key_bits)
    rate = n / (best["kernel_ms"] * 1e-3)
    return {"keys": n, "unique": n_unique, "k": k, "key_bits": key_bits, "passes": (key_bits + 7) // 8, "steps": args.steps,
            "kernel_ms": best["kernel_ms"], "sort_ms": best["sort"], "run_heads_ms": best["run_heads"], "emit_ms": best["emit"],
            "call_wall_ms": min(r["wall_ms"] for r in runs), "kernel_ms_all": [r["kernel_ms"] for r in runs],
            "keys_per_s": rate, "model_bytes_per_key": bpk, "model_bytes_per_s": rate * bpk,
            "frac_of_8TBps_peak": rate * bpk / PEAK_BYTES_PER_S, "store_ceiling_bytes_per_s": bw.value,
            "host_np_unique": {"keys": m, "seconds": host_s, "keys_per_s": m / host_s, "equal_to_device": prefix_equal},
            "generate_sequence_s": t_gen}


def step_lookup(args):
    import numpy as np
    from graph_kmer_index_amd import _lib
    from graph_kmer_index_amd.kmer_counter import DeviceCounter, unique_counts_on_device
    lib = _lib.load()
    _lib.require_device()
    k, key_bits = args.k, 2 * args.k
    dflat, _ = reference_kmers(int(args.bases), k, args.threads)
    n = dflat.n
    u, c = unique_counts_on_device(dflat.hashes.view(0, n), 1, key_bits)
    counter = DeviceCounter(u, c, key_bits)
    n_unique = u.n
    q = min(n, int(args.queries))
    present = dflat.hashes.view(0, q)                    # the reference's own k-mers, in sequence order: all present
    rng = np.random.default_rng(99)
    absent = _lib.DeviceArray.from_host(rng.integers(0, 1 << key_bits, size=q, dtype=np.uint64))
    out = {}
    for name, d_q in (("present", present), ("random", absent)):
        best = None
        for _ in range(3):
            _lib.check(lib.gki_device_synchronize())
            t0 = time.perf_counter()
            d_out = counter.lookup_on_device(d_q)
            dt = time.perf_counter() - t0
            hits = int(np.count_nonzero(d_out.to_host(min(q, 1 << 22))))
            d_out.free()
            best = dt if best is None else min(best, dt)
        out[name] = {"queries": q, "seconds": best, "lookups_per_s": q / best, "hits_in_first_4M": hits}
    rate = C.c_double(0.0)
    _lib.check(lib.gki_measure_random_loads(2 << 30, 1 << 31, C.byref(rate)))
    absent.free()
    counter.free()
    dflat.free()
    return {"unique": n_unique, "lookup": out, "random_loads_per_s": rate.value,
            "what": "wall time of gki_counter_lookup (launch + synchronise), best of three"}


STEPS = {"count": (step_count, 480), "lookup": (step_lookup, 360)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=2.5e8)
    ap.add_argument("--k", type=int, default=31)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-prefix", type=float, default=1e7)
    ap.add_argument("--queries", type=float, default=1e8)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=sorted(STEPS), default=None, help="run one step in this process (the tool's children)")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(STEPS[args.step][0](args)))
        return 0
    result = {"bench": "count_kmers", "bases": int(args.bases)}
    for name in ("count", "lookup"):
        cmd = ["timeout", "-k", "10", str(STEPS[name][1]), sys.executable, os.path.abspath(__file__), "--step", name,
               "--bases", repr(args.bases), "--k", str(args.k), "--threads", str(args.threads), "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--host-prefix", repr(args.host_prefix), "--queries", repr(args.queries)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")]
        if p.returncode != 0 or not lines:
            result["failed_step"] = {"name": name, "exit_status": p.returncode}
            print(json.dumps(result))
            return p.returncode or 1                     # nothing more is started on the device after a failure
        result[name] = json.loads(lines[-1][len("RESULT "):])
    text = json.dumps(result)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
