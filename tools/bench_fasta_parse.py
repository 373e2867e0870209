#!/usr/bin/env python3
"""Secondary benchmark (not the headline): a reference FASTA FILE to its records' letters in HBM on one MI355X, host route
against device route, over whole files (nothing is scaled from a prefix).

    python tools/bench_fasta_parse.py [--bases 3e9] [--records 24] [--runs 3] [--dir DIR] [--no-graph-build]

A multi-record reference of --bases random letters, wrapped at 60, is written once as plain text, as BGZF level 6
(bgzf.write_bgzf) and as plain gzip level 6 (several members, none of them BGZF).  Per encoding, --runs times each:
  host     snp_kmer_finder.read_fasta_records (one read of the file, NumPy) and the upload of every record: what a caller
           has when its letters are in HBM
  device   fasta_files.reference_from_file end to end, with its own stage clocks (text = file read + upload + inflate as
           the loop sees them, parse = the three parse calls of every piece, assemble = the device-to-device layout) and
           the parse kernels' device time; the text's own steps -- file read (for gzip this holds the host's inflate),
           upload, inflate with the line cut -- in a pass of their own over the same step functions
  copy     a device-to-device copy of as many bytes as the text has, same process: the parse kernels' time is reported
           as a multiple of it
The device letters are asserted equal to the host route's: names, bounds, the whole array's checksum (sum and xor, on
the device against NumPy) and, once per encoding, every letter after a copy back.  The plain file is
parsed once more as ONE piece, so that the kernels themselves see byte offsets beyond 2^31.  Then tools/bench_graph_build.py is
run with --fasta-parse host and --fasta-parse device.  Prints one JSON object per step."""
import argparse
import gzip
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_graph_build import vcf_text_stages as text_stages                      # noqa: E402
from graph_kmer_index_amd import _lib, bgzf                                      # noqa: E402
from graph_kmer_index_amd.fasta_files import reference_from_file                 # noqa: E402
from graph_kmer_index_amd.snp_kmer_finder import read_fasta_records              # noqa: E402

LETTERS = np.frombuffer(b"ACGT", dtype=np.uint8)
WIDTH = 60


def write_reference(path, n_bases, n_records, seed=77):
    """chr1 .. chrN, sizes falling from the first to the last (the last a third of the first), wrapped at WIDTH."""
    rng = np.random.default_rng(seed)
    weights = np.linspace(3.0, 1.0, n_records)
    sizes = np.floor(weights / weights.sum() * n_bases).astype(np.int64)
    sizes[0] += n_bases - sizes.sum()
    with open(path, "wb") as f:
        for i, size in enumerate(sizes.tolist()):
            f.write(b">chr%d synthetic record %d of %d letters\n" % (i + 1, i + 1, size))
            letters = LETTERS[rng.integers(0, 4, size=size, dtype=np.uint8)]
            whole = size // WIDTH * WIDTH
            rows = np.empty((whole // WIDTH, WIDTH + 1), dtype=np.uint8)
            rows[:, :WIDTH] = letters[:whole].reshape(-1, WIDTH)
            rows[:, WIDTH] = 10
            f.write(rows.tobytes())
            del rows
            if whole < size:
                f.write(letters[whole:].tobytes() + b"\n")
    return sizes


def write_gzip_members(path, data, threads, member_bytes=64 << 20):
    """Plain gzip, level 6, one member per 64 MiB compressed side by side: one serial stream to a reader, not BGZF."""
    from concurrent.futures import ThreadPoolExecutor
    view = memoryview(data)
    with open(path, "wb") as f, ThreadPoolExecutor(threads) as pool:
        f.writelines(pool.map(lambda a: gzip.compress(view[a:a + member_bytes], 6), range(0, len(view), member_bytes)))


def host_checksum(arrays):
    """(sum mod 2^64, xor) of the letters, as DeviceArray.checksum gives them for one-byte elements."""
    total, x = 0, 0
    for a in arrays:
        total = (total + int(a.sum(dtype=np.uint64))) % (1 << 64)
        x ^= int(np.bitwise_xor.reduce(a)) if len(a) else 0
    return total, x


def host_route(path):
    """(seconds of read_fasta_records, seconds of the upload, names, host arrays)."""
    lib = _lib.load()
    t0 = time.perf_counter()
    names, records = read_fasta_records(path)
    t1 = time.perf_counter()
    with _lib.DeviceScope() as s:
        letters = s.array(sum(len(r) for r in records), np.uint8)
        at = 0
        for r in records:
            _lib.check(lib.gki_memcpy_h2d(letters.ptr.value + at, _lib.hptr(r), len(r)))
            at += len(r)
        _lib.check(lib.gki_device_synchronize())
        t2 = time.perf_counter()
    return t1 - t0, t2 - t1, names, records


def device_copy_seconds(n_bytes):
    lib = _lib.load()
    with _lib.DeviceScope() as s:
        a, b = s.array(n_bytes, np.uint8), s.array(n_bytes, np.uint8)
        a.zero()
        times = []
        for _ in range(3):
            _lib.check(lib.gki_device_synchronize())
            t0 = time.perf_counter()
            _lib.check(lib.gki_memcpy_d2d(b.ptr, a.ptr, n_bytes))
            _lib.check(lib.gki_device_synchronize())
            times.append(time.perf_counter() - t0)
    return statistics.median(times)


def spread(values):
    return {"median": round(statistics.median(values), 4), "min": round(min(values), 4), "max": round(max(values), 4)}


def measure(path, runs, text_bytes, one_piece=False):
    out = {"file_bytes": os.path.getsize(path)}
    host = []
    for _ in range(runs):
        names = records = None                            # one set of host arrays at a time
        read_s, upload_s, names, records = host_route(path)
        host.append((read_s, upload_s))
    want_bounds = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.int64)
    want_sum = host_checksum(records)
    out["host"] = {"read_fasta_records": spread([h[0] for h in host]), "upload": spread([h[1] for h in host]),
                   "whole": spread([h[0] + h[1] for h in host])}
    del host
    device = []
    for i in range(runs):
        t0 = time.perf_counter()
        ref = reference_from_file(path)
        whole = time.perf_counter() - t0
        assert ref.names == names and ref.records_in_file == names, "names differ"
        assert np.array_equal(ref.bounds, want_bounds), "bounds differ"
        assert ref.letters.checksum() == want_sum, "the letters' checksum differs"
        if i == 0:
            got = ref.to_host()
            assert all(np.array_equal(g, r) for g, r in zip(got, records)), "letters differ"
            del got
        device.append(dict(ref.timings, whole=whole))
        ref.free()
    if one_piece:                                         # the whole text as ONE piece: byte offsets beyond 2^31 in the kernels
        ref = reference_from_file(path, chunk_bytes=text_bytes + 1)
        assert ref.names == names and np.array_equal(ref.bounds, want_bounds), "one piece: names or bounds differ"
        assert ref.letters.checksum() == want_sum, "one piece: the letters' checksum differs"
        assert np.array_equal(ref.record(len(names) - 1).to_host(), records[-1]), "one piece: the last record differs"
        out["one_piece_of_bytes"] = text_bytes
        out["one_piece_parse_kernel_ms"] = round(ref.timings["parse_kernel_ms"], 3)
        ref.free()
    del records
    out["device"] = {k: spread([d[k] for d in device]) for k in device[0]}
    out["letters"] = int(want_bounds[-1])
    out["offsets_beyond_2_31"] = bool(want_bounds[-1] > 2 ** 31)
    stages = [text_stages(path) for _ in range(runs)]
    out["device_text_stages"] = {k.replace("vcf_", ""): spread([s[k] for s in stages]) for k in stages[0]}
    copy = device_copy_seconds(min(text_bytes, 4 << 30))
    out["device_copy_of_text_bytes_ms"] = round(copy * 1e3 * text_bytes / min(text_bytes, 4 << 30), 3)
    out["parse_kernels_over_copy"] = round(out["device"]["parse_kernel_ms"]["median"] / out["device_copy_of_text_bytes_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=3e9)
    ap.add_argument("--records", type=int, default=24)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--dir", default=None, help="where the input files go (default: a temporary directory)")
    ap.add_argument("--no-graph-build", action="store_true")
    args = ap.parse_args()
    _lib.require_device()
    with tempfile.TemporaryDirectory(prefix="gki_fasta_parse_", dir=args.dir) as d:
        paths = {"plain": os.path.join(d, "ref.fa"), "bgzf": os.path.join(d, "ref_bgzf.fa.gz"),
                 "gzip": os.path.join(d, "ref_gzip.fa.gz")}
        t0 = time.perf_counter()
        write_reference(paths["plain"], int(args.bases), args.records)
        with open(paths["plain"], "rb") as f:
            data = f.read()
        bgzf.write_bgzf(paths["bgzf"], data, threads=args.threads)
        write_gzip_members(paths["gzip"], data, args.threads)
        text_bytes = len(data)
        del data
        print("wrote the input files in %.0f s" % (time.perf_counter() - t0), flush=True)
        reference_from_file(paths["plain"], ["chr%d" % args.records]).free()          # warms the pool and the library
        for encoding in ("plain", "bgzf", "gzip"):
            print(json.dumps({encoding: measure(paths[encoding], args.runs, text_bytes, encoding == "plain")}), flush=True)
    if not args.no_graph_build:
        for route in ("host", "device"):
            print("bench_graph_build.py --fasta-parse %s" % route, flush=True)
            subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_graph_build.py"), "--bases", str(args.bases),
                            "--runs", str(args.runs), "--fasta-parse", route] + (["--dir", args.dir] if args.dir else []),
                           check=True)


if __name__ == "__main__":
    main()
